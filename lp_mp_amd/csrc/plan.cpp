// plan.cpp — see plan.hpp.  Host restatement of the reference's ordering / weight rules, plus the
// level scheduling that makes the Gauss-Seidel sweep executable as a few wide kernel launches.
#include "plan.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <stdexcept>
#include <thread>

namespace lpmp {

namespace {

// Contiguous chunks of [0, n) on up to LPMP_PLAN_THREADS (default: the hardware's, at most 16) threads; small ranges run on the
// caller's thread.  The analysis below is a handful of linear passes over millions of updates: the two that build the
// op records and the packets are independent per update / per record.  An exception of any chunk is rethrown.
constexpr int PLAN_MAX_THREADS = 64;
template <class F>
void parallel_chunks(int64_t n, int64_t min_per_thread, F&& f) {
  static const int max_threads = [] {
    const char* e = std::getenv("LPMP_PLAN_THREADS");
    const int hw = (int)std::thread::hardware_concurrency();
    // (the per-thread scratch of the callers below has PLAN_MAX_THREADS slots: the thread index never exceeds it)
    return std::max(1, std::min(PLAN_MAX_THREADS, e ? std::atoi(e) : std::min(16, hw > 0 ? hw : 1)));
  }();
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(max_threads, n / std::max<int64_t>(1, min_per_thread)));
  if (nt <= 1) { f((int64_t)0, n, 0); return; }
  std::vector<std::thread> th;
  std::vector<std::exception_ptr> err((size_t)nt);
  th.reserve((size_t)nt);
  auto work = [&](int t) { try { f(n * t / nt, n * (t + 1) / nt, t); } catch (...) { err[(size_t)t] = std::current_exception(); } };
  int started = 0;
  try {
    for (; started < nt - 1; ++started) th.emplace_back(work, started);
  } catch (...) {}                                   // (no more threads to be had: the caller's thread takes the rest, chunk by chunk)
  for (int t = started; t < nt; ++t) work(t);
  for (auto& x : th) x.join();
  for (auto& e : err) if (e) std::rethrow_exception(e);
}

// message_passing_schedule -> what each side does (reference factors_messages.hxx:1530-1545)
struct SchedCaps { bool to_left, to_right, from_left, from_right; };
SchedCaps caps(int s) {
  switch (s) {
    case LPMP_SCHED_LEFT: return {false, true, false, true};
    case LPMP_SCHED_RIGHT: return {true, false, true, false};
    case LPMP_SCHED_FULL: return {true, true, true, true};
    case LPMP_SCHED_ONLY_SEND: return {true, true, false, false};
    default: return {false, false, false, false};
  }
}

[[noreturn]] void fail(const std::string& s) { throw std::runtime_error(s); }

// reference topological_sort.hxx:100-144 — DFS, roots by index, successors by insertion, reversed post-order
std::vector<int32_t> reference_topological_order(int64_t nf, const int32_t* rel, int64_t n_rel) {
  std::vector<int64_t> head(nf + 1, 0);
  for (int64_t i = 0; i < n_rel; ++i) {
    const int32_t a = rel[2 * i], b = rel[2 * i + 1];
    if (a < 0 || a >= nf || b < 0 || b >= nf) fail("factor relation out of range");
    head[a + 1]++;
  }
  std::partial_sum(head.begin(), head.end(), head.begin());
  std::vector<int32_t> succ(n_rel);
  {
    std::vector<int64_t> cur(head.begin(), head.end() - 1);
    for (int64_t i = 0; i < n_rel; ++i) succ[cur[rel[2 * i]]++] = rel[2 * i + 1];
  }
  std::vector<uint8_t> seen(nf, 0);
  std::vector<int32_t> post;
  post.reserve(nf);
  struct Frame { int32_t node; int64_t next; };
  std::vector<Frame> st;
  for (int64_t root = 0; root < nf; ++root) {
    if (seen[root]) continue;
    seen[root] = 1;
    st.push_back({(int32_t)root, head[root]});
    while (!st.empty()) {
      Frame& fr = st.back();
      const int64_t end = head[fr.node + 1];
      while (fr.next != end && seen[succ[fr.next]]) ++fr.next;
      if (fr.next == end) {
        post.push_back(fr.node);
        st.pop_back();
      } else {
        const int32_t nx = succ[fr.next++];
        seen[nx] = 1;
        st.push_back({nx, head[nx]});
      }
    }
  }
  std::reverse(post.begin(), post.end());
  return post;
}

}  // namespace

void diff_band(const double* D, int64_t n, int32_t* lo, int32_t* hi) {
  auto bits = [&](int64_t k) { uint64_t b; std::memcpy(&b, D + k, sizeof b); return b; };
  int64_t l = 0, h = n - 1;
  while (l < n && bits(l) == bits(0)) ++l;
  while (h >= l && bits(h) == bits(n - 1)) --h;
  *lo = (int32_t)l; *hi = (int32_t)h;
}

bool Plan::diff_launch_banded(const int32_t* tabs, int64_t n) const {
  if (no_diff_band) return false;
  for (int64_t j = 0; j < n; ++j) if (sh_banded[(size_t)tabs[j]] != 1) return false;
  return true;
}

bool Plan::diff_launch_shift_banded(const int32_t* tabs, const int32_t* ne, int64_t n) const {
  if (no_diff_band) return false;
  for (int64_t j = 0; j < n; ++j) if (!diff_band_rule(sh_lo[(size_t)tabs[j]], sh_hi[(size_t)tabs[j]], ne[j])) return false;
  return true;
}

bool Plan::refresh_diff_band(std::vector<LevelRange>& launches, const std::vector<int32_t>& tabs_off, const std::vector<int32_t>& tabs,
                             const std::vector<int32_t>& tabs_ne) const {
  bool changed = false;
  for (LevelRange& lr : launches) {
    if (lr.kclass != KC_DIFF || lr.diff_row < 0 || (size_t)lr.diff_row + 1 >= tabs_off.size()) continue;
    const int32_t t0 = tabs_off[(size_t)lr.diff_row], t1 = tabs_off[(size_t)lr.diff_row + 1];
    const bool band = !lr.diff_shift && diff_launch_banded(tabs.data() + t0, t1 - t0);
    const bool shift_band = lr.diff_shift && tabs_ne.size() == tabs.size() && diff_launch_shift_banded(tabs.data() + t0, tabs_ne.data() + t0, t1 - t0);
    changed = changed || band != lr.diff_band || shift_band != lr.diff_shift_band;
    lr.diff_band = band; lr.diff_shift_band = shift_band;
  }
  return changed;
}

void Plan::set_shared_pool(const double* values) {
  if (!values) fail("shared pool: null argument");
  if (n_shared <= 0) fail("shared pool: the model has no pool of shared tables");
  for (int t = 0; t < n_shared; ++t)       // (refused for the reason build() gives, before anything is changed)
    for (int64_t i = sh_off[(size_t)t]; i < sh_off[(size_t)t + 1]; ++i)
      if (values[i] != values[i]) fail("shared table " + std::to_string(t) + ": NaN entry");
  sh_data.assign(values, values + sh_off[(size_t)n_shared]);
  for (int t = 0; t < n_shared; ++t) {
    if (sh_banded[(size_t)t] < 0 && !sh_shift_ref[(size_t)t]) continue;   // neither a DIFF nor a DIFF_SHIFT factor references the entry
    diff_band(sh_data.data() + sh_off[(size_t)t], sh_dim1[(size_t)t], &sh_lo[(size_t)t], &sh_hi[(size_t)t]);
    if (sh_banded[(size_t)t] >= 0) sh_banded[(size_t)t] = diff_band_rule(sh_lo[(size_t)t], sh_hi[(size_t)t], sh_dim1[(size_t)t]) ? 1 : 0;
  }
}

void Plan::build(const lpmp_model& m) {
  const bool timed_ = std::getenv("LPMP_PLAN_TIMES") != nullptr;
  auto t_last_ = std::chrono::steady_clock::now();
  auto lap_ = [&](const char* what) { if (!timed_) return; const auto now = std::chrono::steady_clock::now(); std::fprintf(stderr, "lpmp: plan build %-10s %.0f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last_).count()); t_last_ = now; };
  if (m.n_ftypes <= 0 || m.n_factors <= 0) fail("model has no factors");
  if (m.n_factors > std::numeric_limits<int32_t>::max() || m.n_messages > std::numeric_limits<int32_t>::max() / 2)
    fail("model too large for 32-bit factor/message indices");
  n_ftypes = m.n_ftypes; n_mtypes = m.n_mtypes; n_tables = m.n_tables;
  ftype_primal.assign(n_ftypes, 0);
  if (m.ftype_computes_primal) ftype_primal.assign(m.ftype_computes_primal, m.ftype_computes_primal + n_ftypes);
  mtypes.assign(m.mtypes, m.mtypes + n_mtypes);
  if (n_tables < 0) fail("negative table count");
  if (n_tables > 0) {
    if (!m.tab_off || !m.tab_data || !m.tab_nleft) fail("labeling tables missing");
    tab_off.assign(m.tab_off, m.tab_off + n_tables + 1);
    tab_data.assign(m.tab_data, m.tab_data + tab_off[n_tables]);
    tab_nleft.assign(m.tab_nleft, m.tab_nleft + n_tables);
    // an entry indexes the left factor's labelings (tab_nleft = "no matching left labeling"): anything else would be
    // an out-of-bounds access in the labeling receive / send kernels
    if (tab_off[0] != 0) fail("labeling tables: tab_off must start at 0");
    for (int t = 0; t < n_tables; ++t) {
      if (tab_off[t + 1] < tab_off[t] || tab_nleft[t] <= 0) fail("labeling table " + std::to_string(t) + ": bad offsets / left labeling count");
      for (int64_t j = tab_off[t]; j < tab_off[t + 1]; ++j)
        if (tab_data[j] < 0 || tab_data[j] > tab_nleft[t]) fail("labeling table " + std::to_string(t) + ": entry out of range");
    }
  }
  nf = m.n_factors; nm = m.n_messages; constant = m.constant;
  f_type.assign(m.f_type, m.f_type + nf);
  f_kind.assign(m.f_kind, m.f_kind + nf);
  if (m.f_flags) f_flags.assign(m.f_flags, m.f_flags + nf); else f_flags.assign(nf, 0);
  f_dim0.assign(m.f_dim0, m.f_dim0 + nf);
  if (m.f_dim1) f_dim1.assign(m.f_dim1, m.f_dim1 + nf); else f_dim1.assign(nf, 0);
  f_coff.assign(nf + 1, 0); f_doff.assign(nf + 1, 0);
  // the pool of shared pairwise tables
  n_shared = m.n_shared_tables;
  if (n_shared < 0) fail("negative shared table count");
  sh_off.clear(); sh_dim0.clear(); sh_dim1.clear(); sh_data.clear(); f_table.clear();
  if (n_shared > 0) {
    if (!m.sh_off || !m.sh_dim0 || !m.sh_dim1 || !m.sh_data) fail("shared tables missing");
    sh_off.assign(m.sh_off, m.sh_off + n_shared + 1);
    sh_dim0.assign(m.sh_dim0, m.sh_dim0 + n_shared);
    sh_dim1.assign(m.sh_dim1, m.sh_dim1 + n_shared);
    if (sh_off[0] != 0) fail("shared tables: sh_off must start at 0");
    for (int t = 0; t < n_shared; ++t)
      if (sh_dim0[t] <= 0 || sh_dim1[t] <= 0 || sh_off[t + 1] - sh_off[t] != (int64_t)sh_dim0[t] * sh_dim1[t])
        fail("shared table " + std::to_string(t) + ": bad dimensions / offsets");
    sh_data.assign(m.sh_data, m.sh_data + sh_off[n_shared]);
    // the shared classes pad their LDS tables with NaN and rely on fmin dropping it: a NaN entry of the caller's would vanish there
    // and propagate on the generic kernels — refused here, where the pool is on the host
    for (int t = 0; t < n_shared; ++t)
      for (int64_t i = sh_off[t]; i < sh_off[t + 1]; ++i)
        if (sh_data[(size_t)i] != sh_data[(size_t)i]) fail("shared table " + std::to_string(t) + ": NaN entry");
  }
  sh_lo.assign((size_t)n_shared, 0); sh_hi.assign((size_t)n_shared, -1); sh_banded.assign((size_t)n_shared, -1); sh_shift_ref.assign((size_t)n_shared, 0);
  no_diff_band = std::getenv("LPMP_NO_DIFF_BAND") != nullptr;
  max_dual = 1;
  for (int64_t f = 0; f < nf; ++f) {
    if (f_kind[f] > LPMP_F_PAIRWISE_DIFF && f_kind[f] != LPMP_F_PAIRWISE_DIFF_SHIFT) fail("factor " + std::to_string(f) + ": unknown kind");
    if (f_kind[f] == LPMP_F_PAIRWISE_SHARED) {
      if (f_table.empty()) f_table.assign(nf, -1);
      if (!m.f_table) fail("factor " + std::to_string(f) + ": shared pairwise factor, but the model has no f_table");
      const int32_t t = m.f_table[f];
      if (t < 0 || t >= n_shared) fail("factor " + std::to_string(f) + ": shared table index " + std::to_string(t) + " out of range");
      if (f_dim0[f] != sh_dim0[t] || f_dim1[f] != sh_dim1[t])
        fail("factor " + std::to_string(f) + ": dims " + std::to_string(f_dim0[f]) + " x " + std::to_string(f_dim1[f]) + " do not match shared table " +
             std::to_string(t) + " (" + std::to_string(sh_dim0[t]) + " x " + std::to_string(sh_dim1[t]) + ")");
      f_table[f] = t;
    }
    if (f_kind[f] == LPMP_F_PAIRWISE_DIFF) {            // D = a 1 x (dim0 + dim1 - 1) entry of the same pool
      if (f_table.empty()) f_table.assign(nf, -1);
      if (!m.f_table) fail("factor " + std::to_string(f) + ": difference-indexed pairwise factor, but the model has no f_table");
      const int32_t t = m.f_table[f];
      if (t < 0 || t >= n_shared) fail("factor " + std::to_string(f) + ": shared table index " + std::to_string(t) + " out of range");
      if (f_dim1[f] <= 0) fail("factor " + std::to_string(f) + ": bad dimension");
      if (sh_dim0[t] != 1 || (int64_t)sh_dim1[t] != (int64_t)f_dim0[f] + f_dim1[f] - 1)
        fail("factor " + std::to_string(f) + ": dims " + std::to_string(f_dim0[f]) + " x " + std::to_string(f_dim1[f]) + " need a difference vector of 1 x " +
             std::to_string((int64_t)f_dim0[f] + f_dim1[f] - 1) + ", shared table " + std::to_string(t) + " is " + std::to_string(sh_dim0[t]) + " x " + std::to_string(sh_dim1[t]));
      f_table[f] = t;
      if (sh_banded[(size_t)t] < 0) {
        if (!sh_shift_ref[(size_t)t]) diff_band(sh_data.data() + sh_off[(size_t)t], sh_dim1[(size_t)t], &sh_lo[(size_t)t], &sh_hi[(size_t)t]);
        sh_banded[(size_t)t] = diff_band_rule(sh_lo[(size_t)t], sh_hi[(size_t)t], sh_dim1[(size_t)t]) ? 1 : 0;
      }
    }
    if (f_kind[f] == LPMP_F_PAIRWISE_DIFF_SHIFT) {      // D = a 1 x n entry of the same pool, any n >= 1; the shift is a cost and is not read
      if (f_table.empty()) f_table.assign(nf, -1);
      if (!m.f_table) fail("factor " + std::to_string(f) + ": shifted difference-indexed pairwise factor, but the model has no f_table");
      const int32_t t = m.f_table[f];
      if (t < 0 || t >= n_shared) fail("factor " + std::to_string(f) + ": shared table index " + std::to_string(t) + " out of range");
      if (f_dim1[f] <= 0) fail("factor " + std::to_string(f) + ": bad dimension");
      if (sh_dim0[t] != 1)
        fail("factor " + std::to_string(f) + ": a shifted difference-indexed factor needs a vector (1 x n), shared table " + std::to_string(t) + " is " +
             std::to_string(sh_dim0[t]) + " x " + std::to_string(sh_dim1[t]));
      f_table[f] = t;
      // the band of D for the shifted banded kernel (sh_banded stays as it is: the plain rule is about DIFF factors only)
      if (sh_banded[(size_t)t] < 0 && !sh_shift_ref[(size_t)t]) diff_band(sh_data.data() + sh_off[(size_t)t], sh_dim1[(size_t)t], &sh_lo[(size_t)t], &sh_hi[(size_t)t]);
      sh_shift_ref[(size_t)t] = 1;
    }
    if (f_type[f] < 0 || f_type[f] >= n_ftypes) fail("factor " + std::to_string(f) + ": type out of range");
    if (f_dim0[f] <= 0 || (f_kind[f] == LPMP_F_PAIRWISE_DENSE && f_dim1[f] <= 0)) fail("factor " + std::to_string(f) + ": bad dimension");
    if (f_kind[f] == LPMP_F_PAIRWISE_POTTS) f_dim1[f] = f_dim0[f];
    if (f_kind[f] == LPMP_F_VECTOR) f_dim1[f] = 0;
    f_coff[f + 1] = f_coff[f] + lpmp_factor_const_size(f_kind[f], f_dim0[f], f_dim1[f]);
    const int64_t ds = lpmp_factor_dual_size(f_kind[f], f_dim0[f], f_dim1[f]);
    f_doff[f + 1] = f_doff[f] + ds;
    max_dual = std::max<int64_t>(max_dual, ds);
  }
  if (m.n_part_pairs < 0 || (m.n_part_pairs > 0 && !m.part_pairs)) fail("partition pairs missing");
  part_pairs.assign(m.part_pairs, m.part_pairs + 2 * m.n_part_pairs);
  for (int32_t x : part_pairs) if (x < 0 || x >= nf) fail("put_in_same_partition: factor out of range");
  part = Partition();
  m_type.assign(m.m_type, m.m_type + nm);
  m_left.assign(m.m_left, m.m_left + nm);
  m_right.assign(m.m_right, m.m_right + nm);
  any_batch = false;
  for (int t = 0; t < n_mtypes; ++t) {
    const auto& mt = mtypes[t];
    if (mt.flags & ~(LPMP_MF_IMPROVEMENT | LPMP_MF_BATCH_TO_RIGHT | LPMP_MF_BATCH_TO_LEFT)) fail("message type " + std::to_string(t) + ": unknown flags");
    any_batch = any_batch || (mt.flags & (LPMP_MF_BATCH_TO_RIGHT | LPMP_MF_BATCH_TO_LEFT)) != 0;
    if (mt.left_ftype < 0 || mt.left_ftype >= n_ftypes || mt.right_ftype < 0 || mt.right_ftype >= n_ftypes)
      fail("message type " + std::to_string(t) + ": factor type out of range");
    if (mt.schedule < 0 || mt.schedule > LPMP_SCHED_NONE) fail("message type " + std::to_string(t) + ": bad schedule");
    if (mt.kind < 0 || mt.kind > LPMP_M_MINNORM) fail("message type " + std::to_string(t) + ": unknown kind");
  }
  for (int64_t i = 0; i < nm; ++i) {
    const int t = m_type[i];
    const int32_t l = m_left[i], r = m_right[i];
    if (t < 0 || t >= n_mtypes || l < 0 || l >= nf || r < 0 || r >= nf || l == r) fail("message " + std::to_string(i) + ": index out of range");
    const auto& mt = mtypes[t];
    bool ok = f_type[l] == mt.left_ftype && f_type[r] == mt.right_ftype && f_kind[l] == LPMP_F_VECTOR;
    if (ok && mt.kind == LPMP_M_UNARY_PAIRWISE)
      ok = f_kind[r] != LPMP_F_VECTOR && (mt.param == 0 || mt.param == 1) && f_dim0[l] == (mt.param == 0 ? f_dim0[r] : f_dim1[r]);
    if (ok && mt.kind == LPMP_M_LABELING)
      ok = f_kind[r] == LPMP_F_VECTOR && mt.param >= 0 && mt.param < n_tables && tab_nleft[mt.param] == f_dim0[l] &&
           tab_off[mt.param + 1] - tab_off[mt.param] == f_dim0[r];
    if (ok && mt.kind == LPMP_M_MINNORM) ok = f_kind[r] == LPMP_F_VECTOR && f_dim0[r] == f_dim0[l];
    if (!ok) fail("message " + std::to_string(i) + ": factors do not fit the message type");
  }
  lap_("checks");

  // ---- per-factor message lists: dispatcher order = left-role types in MessageList order, then right-role
  std::vector<int32_t> rank_l(n_mtypes), rank_r(n_mtypes);
  for (int k = 0; k < n_ftypes; ++k) {
    int r = 0;
    for (int t = 0; t < n_mtypes; ++t) if (mtypes[t].left_ftype == k) rank_l[t] = r++;
    for (int t = 0; t < n_mtypes; ++t) if (mtypes[t].right_ftype == k) rank_r[t] = r++;
  }
  fm_off.assign(nf + 1, 0);
  for (int64_t i = 0; i < nm; ++i) { fm_off[m_left[i] + 1]++; fm_off[m_right[i] + 1]++; }
  std::partial_sum(fm_off.begin(), fm_off.end(), fm_off.begin());
  fm.resize(2 * nm);
  struct Tmp { int32_t rank; int32_t msg; uint8_t role; };
  std::vector<Tmp> tmp(2 * nm);
  {
    std::vector<int64_t> cur(fm_off.begin(), fm_off.end() - 1);
    for (int64_t i = 0; i < nm; ++i) {   // insertion order inside each factor
      tmp[cur[m_left[i]]++] = {rank_l[m_type[i]], (int32_t)i, 0};
      tmp[cur[m_right[i]]++] = {rank_r[m_type[i]], (int32_t)i, 1};
    }
  }
  updated.assign(nf, 0);
  n_row_sends.assign(nf, 0); n_row_receives.assign(nf, 0);
  lap_("msg lists");
  parallel_chunks(nf, 65536, [&](int64_t f_begin, int64_t f_end, int) {
  for (int64_t f = f_begin; f < f_end; ++f) {
    Tmp* b = tmp.data() + fm_off[f];
    Tmp* e = tmp.data() + fm_off[f + 1];
    std::stable_sort(b, e, [](const Tmp& x, const Tmp& y) { return x.rank < y.rank; });
    for (Tmp* p = b; p != e;) {          // runs of one dispatcher; LIFO storages iterate newest first
      Tmp* q = p;
      while (q != e && q->rank == p->rank) ++q;
      const auto& mt = mtypes[m_type[p->msg]];
      const bool lifo = p->role == 0 ? (mt.n_left == 0 && mt.n_right != 0) : (mt.n_right == 0 && mt.n_left != 0);
      if (lifo) std::reverse(p, q);
      p = q;
    }
    bool upd_f = ftype_primal[f_type[f]] != 0;
    int32_t n_s = 0, n_r = 0;
    for (Tmp* p = b; p != e; ++p) {
      const SchedCaps c = caps(mtypes[m_type[p->msg]].schedule);
      MsgEntry& en = fm[fm_off[f] + (p - b)];
      en.msg = p->msg; en.role = p->role;
      if (p->role == 0) {
        en.adjacent = m_right[p->msg];
        en.sends = c.to_right; en.receives = c.from_right; en.adj_sends = c.to_left; en.adj_receives = c.from_left;
      } else {
        en.adjacent = m_left[p->msg];
        en.sends = c.to_left; en.receives = c.from_left; en.adj_sends = c.to_right; en.adj_receives = c.from_right;
      }
      upd_f = upd_f || en.sends || en.receives;
      n_s += en.sends; n_r += en.receives;
    }
    updated[f] = upd_f;
    n_row_sends[f] = n_s; n_row_receives[f] = n_r;
  }
  });
  lap_("dispatch");

  // ---- orderings
  const int32_t* rels[2] = {m.rel_fwd, m.rel_bwd};
  const int64_t nrels[2] = {m.n_rel_fwd, m.n_rel_bwd};
  parallel_chunks(2, 1, [&](int64_t d_begin, int64_t d_end, int) {       // the two directions are independent
    for (int64_t d = d_begin; d < d_end; ++d) {
      order[d] = reference_topological_order(nf, rels[d], nrels[d]);
      upd[d].clear();
      for (int32_t f : order[d]) if (updated[f]) upd[d].push_back(f);
    }
  });
  lap_("orderings");
}

// rows for the updated members of a list (reference allocate_omega / allocate_receive_mask)
// row_of (optional): per list position its row, -1 for a member that is not updated
static void shape_rows(const Plan& p, const int32_t* list, int64_t n, Csr<double>& om, Csr<uint8_t>& mk, std::vector<int64_t>* row_of = nullptr) {
  om.off.assign(1, 0); mk.off.assign(1, 0);
  if (row_of) row_of->assign((size_t)n, -1);
  for (int64_t i = 0; i < n; ++i) {
    if (!p.updated[list[i]]) continue;
    if (row_of) (*row_of)[(size_t)i] = (int64_t)om.off.size() - 1;
    om.off.push_back(om.off.back() + p.row_sends(list[i]));
    mk.off.push_back(mk.off.back() + p.row_receives(list[i]));
  }
  om.data.assign(om.off.back(), 0.0);
  mk.data.assign(mk.off.back(), 0);
}

// reference LP_MP.h:1232-1415
void Plan::anisotropic_weights(const int32_t* list, int64_t n, Csr<double>& om, Csr<uint8_t>& mk) const {
  constexpr int64_t NONE = -1, INF = std::numeric_limits<int64_t>::max();
  std::vector<int64_t> pos(nf, NONE);
  for (int64_t i = 0; i < n; ++i) {
    if (list[i] < 0 || list[i] >= nf) fail("factor index out of range");
    pos[list[i]] = i;
  }
  std::vector<int64_t> n_later(n, 0), last(n, 0), first(n, INF);
  parallel_chunks(n, 65536, [&](int64_t i_begin, int64_t i_end, int) {       // every member on its own
  for (int64_t i = i_begin; i < i_end; ++i) {
    const int32_t f = list[i];
    for (int64_t j = fm_off[f]; j < fm_off[f + 1]; ++j) {
      const MsgEntry& e = fm[j];
      const int64_t a = pos[e.adjacent];
      if (a != NONE && e.adj_receives && a > i) {
        ++n_later[i];
        last[i] = std::max(last[i], a);
        first[i] = std::min(first[i], a);
      }
    }
  }
  });
  // factors outside the list: only those adjacent to >= 2 members get real values, all others read the
  // value-initialised 0 of the reference's unordered_map::operator[] (LP_MP.h:1283-1303, :1322, :1342)
  std::vector<int64_t> out_min_send, out_max_recv;
  if (n < nf) {
    out_min_send.assign(nf, 0); out_max_recv.assign(nf, 0);
    std::vector<int32_t> touch(nf, 0);
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = fm_off[list[i]]; j < fm_off[list[i] + 1]; ++j)
        if (pos[fm[j].adjacent] == NONE) ++touch[fm[j].adjacent];
    for (int64_t g = 0; g < nf; ++g) {
      if (touch[g] < 2) continue;
      int64_t mn = INF, mx = 0;
      for (int64_t j = fm_off[g]; j < fm_off[g + 1]; ++j) {
        const int64_t a = pos[fm[j].adjacent];
        if (a == NONE) continue;
        if (fm[j].adj_sends) mn = std::min(mn, a);
        if (fm[j].adj_receives) mx = std::max(mx, a);
      }
      out_min_send[g] = mn; out_max_recv[g] = mx;
    }
  }
  std::vector<int64_t> row_of;
  shape_rows(*this, list, n, om, mk, &row_of);
  parallel_chunks(n, 65536, [&](int64_t i_begin, int64_t i_end, int) {       // every row on its own
  for (int64_t i = i_begin; i < i_end; ++i) {
    const int32_t f = list[i];
    const int64_t row = row_of[(size_t)i];
    if (row < 0) continue;
    double* o = om.data.data() + om.off[row];
    uint8_t* r = mk.data.data() + mk.off[row];
    int64_t ns = 0, na = 0, nr = 0;
    for (int64_t j = fm_off[f]; j < fm_off[f + 1]; ++j) {
      const MsgEntry& e = fm[j];
      const int64_t a = pos[e.adjacent];
      if (e.sends) {
        const bool s = a != NONE ? ((i < a && updated[e.adjacent]) || last[a] > i) : (i < out_max_recv[e.adjacent]);
        o[ns++] = s ? 1.0 : 0.0;
        na += s;
      }
      if (e.receives) r[nr++] = a != NONE ? (a < i || first[a] < i) : (out_min_send[e.adjacent] < i);
    }
    if (na > 0) {
      const double w = 1.0 / double(n_later[i] + std::max(na, ns - na));   // srmp_weight, :1397
      for (int64_t k = 0; k < ns; ++k) if (o[k] > 0) o[k] *= w;
    }
  }
  });
}

void Plan::ensure_weights(int mode) {
  if (mode < 0 || mode >= LPMP_REPAM_COUNT) fail("no reparametrization mode set");
  if (have[mode]) return;
  parallel_chunks(2, 1, [&](int64_t d_begin, int64_t d_end, int) {              // the two directions are independent
  for (int64_t d = d_begin; d < d_end; ++d) {
    Csr<double>& om = omega[d][mode];
    Csr<uint8_t>& mk = mask[d][mode];
    const std::vector<int32_t>& ord = order[d];
    if (mode == LPMP_REPAM_ANISOTROPIC) {
      anisotropic_weights(ord.data(), nf, om, mk);
    } else if (mode == LPMP_REPAM_ANISOTROPIC2) {   // reference LP_MP.h:1086-1154
      std::vector<int64_t> inv(nf), later(nf, 0);
      for (int64_t i = 0; i < nf; ++i) inv[ord[i]] = i;
      for (int64_t i = 0; i < nm; ++i) {
        const SchedCaps c = caps(mtypes[m_type[i]].schedule);
        const int64_t il = inv[m_left[i]], ir = inv[m_right[i]];
        if (c.to_right && il < ir) ++later[il];
        if (c.to_left && ir < il) ++later[ir];
      }
      shape_rows(*this, ord.data(), nf, om, mk);
      int64_t row = 0;
      for (int64_t i = 0; i < nf; ++i) {
        const int32_t f = ord[i];
        if (!updated[f]) continue;
        int64_t ks = om.off[row], kr = mk.off[row];
        for (int64_t j = fm_off[f]; j < fm_off[f + 1]; ++j) {
          const int64_t a = inv[fm[j].adjacent];
          if (fm[j].sends) om.data[ks++] = i < a ? 1.0 / double(later[i]) : 0.0;
          if (fm[j].receives) mk.data[kr++] = a < i;
        }
        ++row;
      }
    } else {   // uniform / damped uniform, reference LP_MP.h:1422-1449 with leave_weight 0 / 1, full mask :1489
      const double leave = mode == LPMP_REPAM_DAMPED_UNIFORM ? 1.0 : 0.0;
      shape_rows(*this, ord.data(), nf, om, mk);
      for (int64_t r = 0; r < om.rows(); ++r) {
        const double w = 1.0 / (double(om.off[r + 1] - om.off[r]) + leave);
        std::fill(om.data.begin() + om.off[r], om.data.begin() + om.off[r + 1], w);
      }
      std::fill(mk.data.begin(), mk.data.end(), 1);
    }
  }
  });
  have[mode] = true;
}

// ------------------------------------------------------------------------------------------------
// Level scheduling.  The reference sweep is strictly sequential (LP_MP.h:989-992).  Two updates
// commute exactly when they touch disjoint factors, so update u gets
//   level(u) = 1 + max(level of the latest earlier update that touched u or one of the factors u touches)
// and all updates of one level run concurrently with a result identical to the sequential sweep.
// (tests/test_schedule_hazards_host.py states the claim: test_footprints_are_sufficient_for_the_oracle pins what an update
// reads and writes against the oracle, test_every_planned_schedule_is_hazard_free demands that every conflicting pair of
// every planned schedule is ordered by what the executor enforces.)
//
// Several sweeps can be scheduled as ONE sequence (forward then backward of a pass).  With `fuse`, an
// update u2 that directly follows an update u1 of the SAME factor — nothing else touched anything u2
// touches in between — is folded into u1's record when u1 has no sends: "receive R1; receive R2; send S2
// from the state after the receives" is exactly what running u1 then u2 computes, and the factor's dual
// makes one round trip instead of two (2-colour grids: the receive level of the forward sweep and the
// send level of the backward sweep are the same factors).
//
// make_schedule runs the stages below in order; the chain plans of the result come from chain_plan.cpp.
namespace {

// two ops of one record into the same message vector: the same peer, and the same side of it
inline bool same_vector(const Op& a, const Op& b) { return a.peer_dual == b.peer_dual && ((a.info >> 5) & 1) == ((b.info >> 5) & 1); }

// The per-update arrays the stages share (u = position in the sequence of the segments).  Hundreds of MB at the headline size:
// every stage works on them in place.
struct Updates {
  int64_t N = 0;
  std::vector<int32_t> uf, owner, level;       // factor; the update whose record holds u's ops (u itself unless folded); level
  std::vector<const double*> uom;              // omega row (the effective send weights when some message op batches)
  std::vector<const uint8_t*> umk;             // receive-mask row
  std::vector<double> eff_store;               // (the rows of those effective send weights)
  std::vector<int32_t> n_recv_of, n_send_of;   // active ops accumulated on the owner record
  std::vector<int32_t> nr_of_u, ns_of_u;       // active receives / sends of every single update (its own, not the owner's sum)
  int32_t max_level = 0;
  std::vector<int64_t> op_start;               // [N + 1]: op range of every owner record
  // class flags of the owner records (only ever cleared):
  std::vector<uint8_t> all_dense, all_potts;   // exact classes: every peer L x L, L the own label count
  std::vector<uint8_t> var_dense, var_potts;   // padded classes: runtime dims
  std::vector<uint8_t> up_any;                 // streaming class: dense and Potts peers mixed
  std::vector<uint8_t> small_ok;               // lane-per-factor class: every size <= SMALL_MAXD
  std::vector<uint8_t> pw_right;               // updated dense pairwise factor, every op unary-pairwise with the factor on the right
  std::vector<uint8_t> sh_all;                 // shared classes: every op unary-pairwise to a SHARED peer of dims <= 32, the factor on the left
  std::vector<int32_t> max_dim;                // largest peer table dim of the record
  std::vector<int64_t> rec_bytes;              // algorithmic bytes of the record
  std::vector<int32_t> kclass;                 // kernel class of the record
  std::vector<int32_t> rec_upd;                // [records]: the update each record stands for
  std::vector<uint8_t> df_all;                 // class diff: every op unary-pairwise to a DIFF peer of dims <= BIG_MAX_LABELS, the factor on the left
  std::vector<int32_t> sh_group;               // shared classes: the table-set group of the record inside its level and class (classify)
};

// a COMPUTE_PRIMAL factor is updated even without any active message (FactorUpdated, reference
// factors_messages.hxx:3125-3130): the primal passes round its label
bool is_rec(const Plan& p, const Updates& U, int64_t u) {
  return U.owner[u] == u && (U.n_recv_of[u] + U.n_send_of[u] > 0 || p.ftype_primal[p.f_type[U.uf[u]]]);
}

// the rows of the segments, checked, with the effective send weights of batch-capable message ops
void gather_rows(const Plan& p, const std::vector<Plan::Segment>& segs, Updates& U) {
  int64_t N = 0;
  for (const auto& sg : segs) N += sg.n;
  U.N = N;
  U.uf = std::vector<int32_t>(N); U.owner = std::vector<int32_t>(N); U.level = std::vector<int32_t>(N, 0);
  U.uom = std::vector<const double*>(N);
  U.umk = std::vector<const uint8_t*>(N);
  U.n_recv_of = std::vector<int32_t>(N, 0); U.n_send_of = std::vector<int32_t>(N, 0);
  {
    int64_t u = 0;
    for (const auto& sg : segs)
      for (int64_t i = 0; i < sg.n; ++i, ++u) {
        const int32_t f = sg.factors[i];
        if (f < 0 || f >= p.nf) fail("factor index out of range");
        if (sg.om_off[i + 1] - sg.om_off[i] != p.row_sends(f) || sg.mk_off[i + 1] - sg.mk_off[i] != p.row_receives(f))
          fail("row " + std::to_string(i) + ": omega / receive mask length does not match the factor's messages");
        U.uf[u] = f; U.uom[u] = sg.om + sg.om_off[i]; U.umk[u] = sg.mk + sg.mk_off[i];
      }
  }
  if (N > std::numeric_limits<int32_t>::max()) fail("too many updates for one schedule");
  // batch-capable message ops: the weights the individual sends end up with (CallSendMessages' batch rule)
  if (p.any_batch) {
    size_t total = 0;
    for (int64_t u = 0; u < N; ++u) total += (size_t)p.row_sends(U.uf[u]);
    U.eff_store.resize(total + 1);
    size_t at = 0;
    for (int64_t u = 0; u < N; ++u) {
      const int64_t ns = p.row_sends(U.uf[u]);
      for (int64_t k = 0; k < ns; ++k) if (U.uom[u][k] < 0) fail("negative send weight");
      p.effective_send_weights(U.uf[u], U.uom[u], U.eff_store.data() + at);
      U.uom[u] = U.eff_store.data() + at;
      at += (size_t)ns;
    }
  }
}

// what every update touches, and the level recurrence (with the folding of `fuse`): owner, level, the op counts
void level_recurrence(const Plan& p, bool fuse, Updates& U) {
  const int64_t N = U.N;
  std::vector<int32_t> last_level(p.nf, 0), last_toucher(p.nf, -1), last_update_of(p.nf, -1);
  U.nr_of_u = std::vector<int32_t>(N, 0); U.ns_of_u = std::vector<int32_t>(N, 0);
  int32_t max_level = 0;
  // what every update touches (its own factor first, then the peers of its active messages) — independent per update, so the
  // walk over the message lists and the weight / mask rows runs on the planner's threads; the recurrence over the levels below
  // is sequential by nature and only chases these lists
  std::vector<int64_t> t_off((size_t)N + 1, 0);
  parallel_chunks(N, 65536, [&](int64_t u_begin, int64_t u_end, int) {
    for (int64_t u = u_begin; u < u_end; ++u) {
      const int32_t f = U.uf[u];
      int32_t nr = 0, ns = 0; int64_t nt = 1;
      int64_t ks = 0, kr = 0;
      const bool all = p.ftype_primal[p.f_type[f]] && p.f_kind[f] != LPMP_F_VECTOR;
      for (int64_t j = p.fm_off[f]; j < p.fm_off[f + 1]; ++j) {
        const MsgEntry& e = p.fm[j];
        bool active = false;
        if (e.receives && U.umk[u][kr++]) { active = true; ++nr; }
        if (e.sends) { const double w = U.uom[u][ks++]; if (w < 0) fail("negative send weight"); if (w != 0.0) { active = true; ++ns; } }
        if (active || all) ++nt;
      }
      U.nr_of_u[u] = nr; U.ns_of_u[u] = ns; t_off[(size_t)u + 1] = nt;
    }
  });
  for (int64_t u = 0; u < N; ++u) t_off[(size_t)u + 1] += t_off[(size_t)u];
  std::vector<int32_t, default_init_allocator<int32_t>> t_data((size_t)t_off[(size_t)N]);
  parallel_chunks(N, 65536, [&](int64_t u_begin, int64_t u_end, int) {
    for (int64_t u = u_begin; u < u_end; ++u) {
      const int32_t f = U.uf[u];
      int32_t* out_t = t_data.data() + t_off[(size_t)u];
      *out_t++ = f;
      int64_t ks = 0, kr = 0;
      // a pairwise factor that rounds itself reads and writes the labels of ALL its unaries in a primal pass
      // (engine.cpp, ensure_primal), whether or not the message is active in this sweep
      const bool all = p.ftype_primal[p.f_type[f]] && p.f_kind[f] != LPMP_F_VECTOR;
      for (int64_t j = p.fm_off[f]; j < p.fm_off[f + 1]; ++j) {
        const MsgEntry& e = p.fm[j];
        bool active = false;
        if (e.receives && U.umk[u][kr++]) active = true;
        if (e.sends && U.uom[u][ks++] != 0.0) active = true;
        if (active || all) *out_t++ = e.adjacent;
      }
    }
  });
  struct Touched { const int32_t* b; const int32_t* e; const int32_t* begin() const { return b; } const int32_t* end() const { return e; } };
  std::vector<int32_t>& owner = U.owner;
  std::vector<int32_t>& level = U.level;
  std::vector<int32_t>& n_recv_of = U.n_recv_of;
  std::vector<int32_t>& n_send_of = U.n_send_of;
  for (int64_t u = 0; u < N; ++u) {
    const int32_t f = U.uf[u];
    const Touched touched{t_data.data() + t_off[(size_t)u], t_data.data() + t_off[(size_t)u + 1]};
    const int32_t nr = U.nr_of_u[u], ns = U.ns_of_u[u];
    int32_t lv = 0;
    for (int32_t g : touched) lv = std::max(lv, last_level[g]);
    const int32_t prev = last_update_of[f];
    // u2 must not receive: the packed kernels request the vectors of several receives of a record at once, so a
    // record may not receive through the same message twice (forward and backward masks can both select it)
    bool merge = fuse && prev >= 0 && nr == 0 && ns > 0 && n_send_of[prev] == 0 && level[prev] == lv &&
                 n_recv_of[prev] + ns <= 32000;
    if (merge)
      for (int32_t g : touched)
        if (last_level[g] == lv && last_toucher[g] != prev) { merge = false; break; }
    if (merge) {
      owner[u] = prev; level[u] = lv;
      n_recv_of[prev] += nr; n_send_of[prev] += ns;
      for (int32_t g : touched) { last_level[g] = lv; last_toucher[g] = prev; }
    } else {
      owner[u] = (int32_t)u; level[u] = lv + 1;
      n_recv_of[u] = nr; n_send_of[u] = ns;
      max_level = std::max(max_level, level[u]);
      // an update without active ops touches nothing and is dropped, unless its factor type computes a primal:
      // that record stays (it rounds the label in primal passes) and reads / writes its own duals
      if (nr + ns > 0 || p.ftype_primal[p.f_type[f]]) {
        for (int32_t g : touched) { last_level[g] = level[u]; last_toucher[g] = (int32_t)u; }
        last_update_of[f] = (int32_t)u;
      }
    }
  }
  U.max_level = max_level;
}

// records of the owners, ops = all receives of the members (sequence order), then all sends; the per-owner class flags and
// algorithmic bytes.  Returns the algorithmic bytes of the schedule.
int64_t build_ops(const Plan& p, Updates& U, OpVec& ops) {
  const int64_t N = U.N;
  const std::vector<int32_t>& owner = U.owner;
  const std::vector<int32_t>& n_recv_of = U.n_recv_of;
  U.op_start = std::vector<int64_t>(N + 1, 0);
  std::vector<int64_t>& op_start = U.op_start;
  for (int64_t u = 0; u < N; ++u) op_start[u + 1] = op_start[u] + (owner[u] == u ? n_recv_of[u] + U.n_send_of[u] : 0);
  if (op_start[N] > std::numeric_limits<int32_t>::max()) fail("too many active message operations for one schedule");
  ops = OpVec((size_t)op_start[N]);                 // (every slot is written below: the counts are the same walk over the rows)
  // where every update writes inside its owner's op range: receives of the members in sequence order, then the sends
  std::vector<int32_t> r_at(N, 0), s_at(N, 0);
  {
    std::vector<int32_t> cur_r(N, 0), cur_s(N, 0);
    for (int64_t u = 0; u < N; ++u) { const int32_t o = owner[u]; r_at[u] = cur_r[o]; cur_r[o] += U.nr_of_u[u]; s_at[u] = cur_s[o]; cur_s[o] += U.ns_of_u[u]; }
  }
  U.rec_bytes = std::vector<int64_t>(N, 0);
  U.all_dense = std::vector<uint8_t>(N, 1); U.all_potts = std::vector<uint8_t>(N, 1);
  U.var_dense = std::vector<uint8_t>(N, 1); U.var_potts = std::vector<uint8_t>(N, 1);
  U.up_any = std::vector<uint8_t>(N, 1);
  U.small_ok = std::vector<uint8_t>(N, 1);
  U.pw_right = std::vector<uint8_t>(N, 1);
  U.sh_all = std::vector<uint8_t>(N, 1);
  U.df_all = std::vector<uint8_t>(N, 1);
  U.max_dim = std::vector<int32_t>(N, 0);
  std::vector<uint8_t>& all_dense = U.all_dense; std::vector<uint8_t>& all_potts = U.all_potts;
  std::vector<uint8_t>& var_dense = U.var_dense; std::vector<uint8_t>& var_potts = U.var_potts;
  std::vector<uint8_t>& up_any = U.up_any; std::vector<uint8_t>& small_ok = U.small_ok; std::vector<uint8_t>& pw_right = U.pw_right;
  std::vector<uint8_t>& sh_all = U.sh_all; std::vector<uint8_t>& df_all = U.df_all;
  std::vector<int32_t>& max_dim = U.max_dim;
  std::vector<int64_t> alg_bytes_of_thread(PLAN_MAX_THREADS, 0);
  // (several updates may share an owner record — folded sweeps — and land on different threads: the per-owner flags only
  // ever go from 1 to 0, sums and maxima are atomic)
  auto clear_flag = [](uint8_t& x) { __atomic_store_n(&x, (uint8_t)0, __ATOMIC_RELAXED); };
  auto atomic_max = [](int32_t& x, int32_t v) { int32_t cur = __atomic_load_n(&x, __ATOMIC_RELAXED); while (cur < v && !__atomic_compare_exchange_n(&x, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {} };
  parallel_chunks(N, 65536, [&](int64_t u_begin, int64_t u_end, int thread) {
  int64_t alg_local = 0;
  for (int64_t u = u_begin; u < u_end; ++u) {
    const int32_t f = U.uf[u];
    const int32_t o = owner[u];
    const int32_t own_d0 = p.f_dim0[f];
    if (p.f_doff[f + 1] - p.f_doff[f] > SMALL_MAXD) clear_flag(small_ok[o]);   // also for a record without any op (COMPUTE_PRIMAL types)
    Op* base = ops.data() + op_start[o];
    auto fill = [&](const MsgEntry& e, double w) {
      const auto& mt = p.mtypes[p.m_type[e.msg]];
      const int32_t peer = e.adjacent;
      Op op{};
      op.peer_dual = p.doff(peer);
      op.omega = w;
      op.peer = peer;
      op.len = p.f_dim0[p.m_left[e.msg]];
      op.pd0 = p.f_dim0[peer]; op.pd1 = p.f_dim1[peer];
      const int32_t right = p.m_right[e.msg];
      int side = 0, imp = 0;
      if (mt.kind == LPMP_M_UNARY_PAIRWISE) {
        side = mt.param;
        op.peer_const = e.role == 0 ? p.coff(peer) : -1;
        const bool unary_left = p.f_kind[f] == LPMP_F_VECTOR && e.role == 0;
        if (!(unary_left && p.f_kind[peer] == LPMP_F_PAIRWISE_DENSE && p.f_dim0[peer] == own_d0 && p.f_dim1[peer] == own_d0 && (p.coff(peer) % 2) == 0 &&
              (!p.tables_f32 || (p.f_coff[peer] % 2) == 0))) clear_flag(all_dense[o]);   // (float tables all start 16-byte aligned: the class stays the f64 model's)
        if (!(unary_left && p.f_kind[peer] == LPMP_F_PAIRWISE_POTTS && p.f_dim0[peer] == own_d0)) clear_flag(all_potts[o]);
        if (!(unary_left && p.f_kind[peer] == LPMP_F_PAIRWISE_DENSE && (side == 0 ? p.f_dim0[peer] : p.f_dim1[peer]) == own_d0)) clear_flag(var_dense[o]);
        if (!(unary_left && p.f_kind[peer] == LPMP_F_PAIRWISE_POTTS && p.f_dim0[peer] == own_d0 && p.f_dim1[peer] == own_d0)) clear_flag(var_potts[o]);
        atomic_max(max_dim[o], std::max(p.f_dim0[peer], p.f_dim1[peer]));
        if (!(unary_left && (p.f_kind[peer] == LPMP_F_PAIRWISE_DENSE || p.f_kind[peer] == LPMP_F_PAIRWISE_POTTS) &&
              (side == 0 ? p.f_dim0[peer] : p.f_dim1[peer]) == own_d0)) clear_flag(up_any[o]);
        if (!(unary_left && p.f_kind[peer] == LPMP_F_PAIRWISE_SHARED && (side == 0 ? p.f_dim0[peer] : p.f_dim1[peer]) == own_d0 &&
              p.f_dim0[peer] <= 32 && p.f_dim1[peer] <= 32)) clear_flag(sh_all[o]);
        if (!(unary_left && (p.f_kind[peer] == LPMP_F_PAIRWISE_DIFF || p.f_kind[peer] == LPMP_F_PAIRWISE_DIFF_SHIFT) && (side == 0 ? p.f_dim0[peer] : p.f_dim1[peer]) == own_d0 &&
              p.f_dim0[peer] <= BIG_MAX_LABELS && p.f_dim1[peer] <= BIG_MAX_LABELS)) clear_flag(df_all[o]);
      } else {
        clear_flag(sh_all[o]); clear_flag(df_all[o]);
        clear_flag(all_dense[o]); clear_flag(all_potts[o]); clear_flag(var_dense[o]); clear_flag(var_potts[o]); clear_flag(up_any[o]);
        if (mt.kind == LPMP_M_LABELING) {
          op.peer_const = p.tab_off[mt.param];
          op.pd1 = p.tab_nleft[mt.param];
          imp = (p.f_flags[right] & LPMP_FF_IMPLICIT_ORIGIN) ? 1 : 0;
        }
      }
      op.info = mt.kind | (e.role << 4) | (side << 5) | (imp << 6) | ((p.f_flags[peer] & LPMP_FF_IMPLICIT_ORIGIN) ? 1 << 7 : 0) | (p.f_kind[peer] << 8) |
                ((mt.flags & LPMP_MF_IMPROVEMENT) ? OP_HAS_IMPROVEMENT : 0);
      if (std::max(op.len, std::max(op.pd0, op.pd1)) > SMALL_MAXD || p.f_doff[f + 1] - p.f_doff[f] > SMALL_MAXD) clear_flag(small_ok[o]);
      if (!(mt.kind == LPMP_M_UNARY_PAIRWISE && e.role == 1 && p.f_kind[f] != LPMP_F_VECTOR && p.f_kind[f] != LPMP_F_PAIRWISE_SHARED && p.f_kind[f] != LPMP_F_PAIRWISE_DIFF && p.f_kind[f] != LPMP_F_PAIRWISE_DIFF_SHIFT && p.f_kind[peer] == LPMP_F_VECTOR &&
            p.f_dim1[f] > 0 && op.len == (side == 0 ? p.f_dim0[f] : p.f_dim1[f]))) clear_flag(pw_right[o]);
      return op;
    };
    // algorithmic bytes, counted per update as the reference executes it: own dual read + written
    // once, per receive the peer's table and both message vectors read and one written, per send one peer
    // vector read and written
    const int64_t tab_entry_bytes = p.tables_f32 ? 4 : 8;   // a dense table entry as the device stores it
    auto op_bytes = [&](const Op& op, bool recv) -> int64_t {
      const int code = op.info & 15, pk = (op.info >> 8) & 15;
      if (code == LPMP_M_UNARY_PAIRWISE) {
        const int64_t L = op.len;
        // (a SHARED or DIFF peer: its scale; the table is on-chip.  DIFF_SHIFT: scale and shift)
        if (recv) return 24 * L + (pk == LPMP_F_PAIRWISE_DENSE ? tab_entry_bytes * (int64_t)op.pd0 * op.pd1 : pk == LPMP_F_PAIRWISE_DIFF_SHIFT ? 16 :
                                   ((pk == LPMP_F_PAIRWISE_POTTS || pk == LPMP_F_PAIRWISE_SHARED || pk == LPMP_F_PAIRWISE_DIFF) ? 8 : 0));
        return 16 * L;
      }
      return 16 * (int64_t)op.pd0;
    };
    int64_t ks = 0, kr = 0, bytes = 0, n_act = 0;
    int32_t at_r = r_at[u], at_s = n_recv_of[o] + s_at[u];
    for (int64_t j = p.fm_off[f]; j < p.fm_off[f + 1]; ++j) {
      const MsgEntry& e = p.fm[j];
      if (e.receives && U.umk[u][kr++]) { Op op = fill(e, 1.0); bytes += op_bytes(op, true); base[at_r++] = op; ++n_act; }
    }
    for (int64_t j = p.fm_off[f]; j < p.fm_off[f + 1]; ++j) {
      const MsgEntry& e = p.fm[j];
      if (e.sends) { const double w = U.uom[u][ks++]; if (w != 0.0) { Op op = fill(e, w); bytes += op_bytes(op, false); base[at_s++] = op; ++n_act; } }
    }
    if (n_act > 0) bytes += 16 * (p.f_doff[f + 1] - p.f_doff[f]);
    // an updated dense pairwise factor reads its own table once to compute the min-marginals it sends
    if (ks > 0 && (p.f_kind[f] == LPMP_F_PAIRWISE_DENSE || p.f_kind[f] == LPMP_F_PAIRWISE_SHARED || p.f_kind[f] == LPMP_F_PAIRWISE_DIFF || p.f_kind[f] == LPMP_F_PAIRWISE_DIFF_SHIFT)) {   // (SHARED, DIFF: its scale; DIFF_SHIFT: and its shift)
      bool sends_any = false;
      for (int64_t j = 0; j < ks; ++j) if (U.uom[u][j] != 0.0) { sends_any = true; break; }
      if (sends_any) bytes += p.f_kind[f] == LPMP_F_PAIRWISE_DENSE ? tab_entry_bytes * (int64_t)p.f_dim0[f] * p.f_dim1[f] : p.f_kind[f] == LPMP_F_PAIRWISE_DIFF_SHIFT ? 16 : 8;
    }
    __atomic_fetch_add(&U.rec_bytes[o], bytes, __ATOMIC_RELAXED);
    alg_local += bytes;
  }
  alg_bytes_of_thread[(size_t)thread] = alg_local;
  });
  int64_t alg_bytes = 0;
  for (int64_t b : alg_bytes_of_thread) alg_bytes += b;
  return alg_bytes;
}

// the kernel class of every record
void classify(const Plan& p, Updates& U, const OpVec& ops) {
  const int64_t N = U.N;
  // Records with two receives, or two sends, into ONE vector (duplicate messages between the same two factors) need an
  // op-by-op kernel: the packed kernels request a record's vectors before reducing.  They get a class of their own
  // (the streaming / generic / lane-per-factor kernels work op by op), so that one such record does not take its whole
  // launch off the packed kernels.  (Two pairwise factors between the same two variables are NOT this case: their
  // messages go to different vectors.)
  std::vector<uint8_t> dup_vec(N, 0);
  for (int64_t u = 0; u < N; ++u) {
    if (U.owner[u] != u) continue;
    const Op* o = ops.data() + U.op_start[u];
    const int nr = U.n_recv_of[u], ns = U.n_send_of[u];
    for (int a = 0; a < nr && !dup_vec[u]; ++a) for (int b = a + 1; b < nr; ++b) if (same_vector(o[a], o[b])) { dup_vec[u] = 1; break; }
    for (int a = nr; a < nr + ns && !dup_vec[u]; ++a) for (int b = a + 1; b < nr + ns; ++b) if (same_vector(o[a], o[b])) { dup_vec[u] = 1; break; }
  }
  const std::vector<int32_t>& uf = U.uf;
  const std::vector<int32_t>& n_recv_of = U.n_recv_of;
  const std::vector<int32_t>& n_send_of = U.n_send_of;
  const std::vector<uint8_t>& small_ok = U.small_ok;
  const std::vector<uint8_t>& up_any = U.up_any;
  const std::vector<uint8_t>& all_dense = U.all_dense;
  const std::vector<uint8_t>& all_potts = U.all_potts;
  const std::vector<int32_t>& max_dim = U.max_dim;
  auto cls_of = [&](int64_t u) -> int32_t {
    const int d0 = p.f_dim0[uf[u]];
    if (p.force_generic) return small_ok[u] && n_send_of[u] <= SMALL_MAXD ? KC_SMALL : KC_GENERIC;
    if (dup_vec[u] && p.f_kind[uf[u]] == LPMP_F_VECTOR) {
      if (small_ok[u]) return KC_SMALL;
      const int wd = std::max(d0, max_dim[u]);
      return up_any[u] && wd >= 1 && wd <= BIG_MAX_LABELS ? KC_DENSE_BIG : KC_GENERIC;
    }
    if (p.f_kind[uf[u]] != LPMP_F_VECTOR) {                // updated pairwise factors
      if (small_ok[u]) return KC_SMALL;
      const int w = std::max(p.f_dim0[uf[u]], p.f_dim1[uf[u]]);
      // (pw_right is cleared op by op: a record WITHOUT any op — a COMPUTE_PRIMAL pairwise type whose messages are all inactive in
      // this sweep — keeps it whatever its kind, and the packed kernel would read d0 x d1 table entries where a SHARED / DIFF /
      // DIFF_SHIFT factor holds two or four words.  The kind is asked here as well.)
      const int fk = p.f_kind[uf[u]];
      if (U.pw_right[u] && (fk == LPMP_F_PAIRWISE_DENSE || fk == LPMP_F_PAIRWISE_POTTS) && w <= 32 && n_recv_of[u] + n_send_of[u] <= PW_MAX_OPS)
        return KC_PW_4 + (w <= 4 ? 0 : w <= 8 ? 1 : w <= 16 ? 2 : 3);
      return KC_GENERIC;
    }
    // unaries between SHARED pairwise factors only: the shared class of the padded width (more ops than its slab holds, or
    // more than 32 labels: the generic kernels, which know the kind)
    if (U.sh_all[u] && n_recv_of[u] + n_send_of[u] > 0) {
      const int w = std::max(d0, max_dim[u]);
      if (w <= 32 && n_recv_of[u] + n_send_of[u] <= pk_indirect_cap(w <= 4 ? 4 : w <= 8 ? 8 : w <= 16 ? 16 : 32))
        return KC_SHARED_4 + (w <= 4 ? 0 : w <= 8 ? 1 : w <= 16 ? 2 : 3);
      return small_ok[u] ? KC_SMALL : KC_GENERIC;
    }
    // unaries between DIFF pairwise factors only (any label count up to BIG_MAX_LABELS, any number of ops: the kernel works op by
    // op; duplicate vectors were taken above and run on the generic kernels, which know the kind)
    if (U.df_all[u] && n_recv_of[u] + n_send_of[u] > 0) return KC_DIFF;
    const bool pow = d0 == 4 || d0 == 8 || d0 == 16 || d0 == 32;
    // more ops than the LDS slab of a lane group holds (a hub of a random graph: C4 has a few 30-neighbour variables among
    // 2 M): such a RECORD goes to the op-by-op streaming kernel — left in its class it took its whole launch off the packed
    // kernels (21 of C4's 44 launches per pass ran on the unpacked 16-label kernel of the time: 5.5 of 12.6 ms, profiles/r03_c4a_*)
    if (pow && (all_dense[u] || all_potts[u]) && n_recv_of[u] + n_send_of[u] > (all_dense[u] ? pk_dense_cap(d0) : pk_indirect_cap(d0)) && up_any[u]) return KC_DENSE_BIG;
    if (pow && all_dense[u]) return d0 == 4 ? KC_DENSE_4 : d0 == 8 ? KC_DENSE_8 : d0 == 16 ? KC_DENSE_16 : KC_DENSE_32;
    if (pow && all_potts[u]) return d0 == 4 ? KC_POTTS_4 : d0 == 8 ? KC_POTTS_8 : d0 == 16 ? KC_POTTS_16 : KC_POTTS_32;
    const int w = std::max(d0, max_dim[u]);
    if (w < 1) return small_ok[u] ? KC_SMALL : KC_GENERIC;      // no unary-pairwise peer at all
    if (w > 32) return up_any[u] && w <= BIG_MAX_LABELS ? KC_DENSE_BIG : KC_GENERIC;
    const int slot = w <= 4 ? 0 : w <= 8 ? 1 : w <= 16 ? 2 : 3;
    if (U.var_dense[u]) return KC_DENSE_V4 + slot;
    if (U.var_potts[u]) return KC_POTTS_V4 + slot;
    if (up_any[u]) return KC_DENSE_V4 + slot;               // unaries with both dense and Potts edges: Potts tables made up in registers
    return small_ok[u] ? KC_SMALL : KC_GENERIC;
  };
  U.kclass = std::vector<int32_t>(N, KC_GENERIC);
  for (int64_t u = 0; u < N; ++u) if (is_rec(p, U, u)) U.kclass[u] = cls_of(u);
  // A launch of a shared class stages its distinct tables in LDS: at most SHARED_MAX_TABLES.  The shared records of one level
  // and width are therefore split by TABLE SET into up to SHARED_MAX_GROUPS launches: taken in sequence order, a record joins
  // the first group whose tables together with its own stay within the budget, or opens a group; beyond the last group it runs
  // on the generic class (models with hundreds of tables mixed in every level).  bucket() makes one launch per group.
  U.sh_group = std::vector<int32_t>();
  if (p.n_shared > 0) {
    U.sh_group.assign((size_t)N, 0);
    struct TabSet { int n = 0; int32_t t[SHARED_MAX_TABLES]; };
    std::vector<std::vector<TabSet>> sets;          // per (level, width slot), levels that hold a shared record only: its groups
    std::vector<int64_t> set_of((size_t)(U.max_level + 1) * 4, -1);
    for (int64_t u = 0; u < N; ++u) {
      if (!is_rec(p, U, u) || !kc_is_shared(U.kclass[u])) continue;
      int64_t& si = set_of[(size_t)(U.level[u] - 1) * 4 + (U.kclass[u] - KC_SHARED_4)];
      if (si < 0) { si = (int64_t)sets.size(); sets.emplace_back(); }
      std::vector<TabSet>& groups = sets[(size_t)si];
      const Op* o = ops.data() + U.op_start[u];
      int placed = -1;
      for (size_t gi = 0; gi <= groups.size() && placed < 0; ++gi) {
        if (gi == groups.size()) { if (gi == (size_t)SHARED_MAX_GROUPS) break; groups.emplace_back(); }
        TabSet trial = groups[gi];
        bool fits = true;
        for (int k = 0; k < n_recv_of[u] && fits; ++k) {        // (only receives read a table)
          const int32_t t = p.f_table[(size_t)o[k].peer];
          bool have = false;
          for (int q = 0; q < trial.n; ++q) have = have || trial.t[q] == t;
          if (have) continue;
          if (trial.n == SHARED_MAX_TABLES) fits = false; else trial.t[trial.n++] = t;
        }
        if (fits) { groups[gi] = trial; placed = (int)gi; }
      }
      if (placed >= 0) U.sh_group[(size_t)u] = placed; else U.kclass[u] = KC_GENERIC;
    }
  }
}

// bucket the owner records by (level, class) into out.recs and out.launches; updates without any active op are dropped
void bucket(const Plan& p, Updates& U, const OpVec& ops, Schedule& out) {
  const int64_t N = U.N;
  const int32_t max_level = U.max_level;
  const std::vector<int32_t>& level = U.level;
  const std::vector<int32_t>& kclass = U.kclass;
  // compact keys: only the (level, class) pairs that occur (deep schedules have millions of levels)
  static_assert(KC_COUNT <= 32, "class mask");
  std::vector<uint32_t> level_mask(max_level + 1, 0);
  for (int64_t u = 0; u < N; ++u) {
    if (!is_rec(p, U, u)) continue;
    if (U.n_recv_of[u] > 32767 || U.n_send_of[u] > 32767)     // (UpdRec::n_recv / n_send are int16_t)
      throw UnsupportedModel("factor " + std::to_string(U.uf[u]) + " has more than 32767 active receives or sends in one update");
    level_mask[level[u] - 1] |= 1u << kclass[u];
  }
  std::vector<int64_t> level_base(max_level + 1, 0);
  for (int64_t l = 0; l < max_level; ++l) level_base[l + 1] = level_base[l] + __builtin_popcount(level_mask[l]);
  const int64_t n_keys = level_base[max_level];
  auto key = [&](int64_t u) {
    const int64_t l = level[u] - 1;
    return level_base[l] + __builtin_popcount(level_mask[l] & ((1u << kclass[u]) - 1u));
  };
  std::vector<int64_t> key_count(n_keys + 1, 0), key_recv(n_keys, 0), key_send(n_keys, 0), key_bytes(n_keys, 0);
  std::vector<int32_t> key_level(n_keys, 0), key_class(n_keys, 0), key_maxdim(n_keys, 0);
  for (int64_t u = 0; u < N; ++u) {
    if (!is_rec(p, U, u)) continue;
    const int64_t k = key(u);
    ++key_count[k + 1];
    key_level[k] = level[u]; key_class[k] = kclass[u];
    key_recv[k] += U.n_recv_of[u]; key_send[k] += U.n_send_of[u]; key_bytes[k] += U.rec_bytes[u];
    key_maxdim[k] = std::max(key_maxdim[k], std::max(std::max(p.f_dim0[U.uf[u]], p.f_dim1[U.uf[u]]), U.max_dim[u]));
    out.n_recv += U.n_recv_of[u]; out.n_send += U.n_send_of[u];
  }
  std::partial_sum(key_count.begin(), key_count.end(), key_count.begin());
  out.recs.resize(key_count[n_keys]);
  U.rec_upd = std::vector<int32_t>(key_count[n_keys]);
  {
    std::vector<int64_t> cur(key_count.begin(), key_count.end() - 1);
    for (int64_t u = 0; u < N; ++u) {
      if (!is_rec(p, U, u)) continue;
      const int32_t f = U.uf[u];
      UpdRec r{};
      r.dual_off = p.doff(f);
      r.const_off = p.f_kind[f] == LPMP_F_VECTOR ? -1 : p.coff(f);
      r.d0 = p.f_dim0[f]; r.d1 = p.f_dim1[f];
      r.op_begin = (int32_t)U.op_start[u];
      r.n_recv = (int16_t)U.n_recv_of[u]; r.n_send = (int16_t)U.n_send_of[u];
      r.factor = f;
      r.kind_flags = p.f_kind[f] | (p.f_flags[f] << 4) | (p.ftype_primal[p.f_type[f]] ? UPD_PRIMAL : 0);
      U.rec_upd[cur[key(u)]] = (int32_t)u;
      out.recs[cur[key(u)]++] = r;
    }
  }
  out.diff_tab_off.assign(1, 0); out.diff_tab.clear(); out.diff_tab_ne.clear();
  std::vector<int32_t> diff_seen((size_t)p.n_shared, 0);   // 0, or the smallest d0 + d1 - 1 among the launch's references so far
  for (int64_t k = 0; k < n_keys; ++k) {
    LevelRange lr;
    lr.kclass = key_class[k]; lr.begin = key_count[k]; lr.end = key_count[k + 1];
    lr.level = key_level[k];
    lr.n_recv = key_recv[k]; lr.n_send = key_send[k]; lr.bytes = key_bytes[k];
    lr.max_dim = key_maxdim[k];
    if (lr.kclass == KC_DIFF) {
      // the banded kernel: only if every receive of the launch has a banded vector.  A launch without any receive (the first
      // step of a sweep: sends only, the two kernels do the same there) goes by the vectors of its sends, so that a model is
      // on one kernel throughout.  The pool entries asked are kept: new pool values ask them again (Plan::refresh_diff_band).
      for (int64_t i = lr.begin; i < lr.end; ++i) {
        const UpdRec& r = out.recs[(size_t)i];
        const Op* o = ops.data() + r.op_begin;
        const int n_ops = lr.n_recv > 0 ? r.n_recv : r.n_send;
        // a DIFF_SHIFT peer anywhere in the launch (receive or send): a shifted kernel (banded by the rule of its own, below)
        for (int q = 0; q < r.n_recv + r.n_send && !lr.diff_shift; ++q) lr.diff_shift = p.f_kind[(size_t)o[q].peer] == LPMP_F_PAIRWISE_DIFF_SHIFT;
        for (int q = 0; q < n_ops; ++q) {
          const int32_t t = p.f_table[(size_t)o[q].peer];
          const int32_t ne = p.f_dim0[(size_t)o[q].peer] + p.f_dim1[(size_t)o[q].peer] - 1;
          if (!diff_seen[(size_t)t]) { diff_seen[(size_t)t] = ne; out.diff_tab.push_back(t); }
          else diff_seen[(size_t)t] = std::min(diff_seen[(size_t)t], ne);
        }
      }
      const int32_t t0 = out.diff_tab_off.back();
      std::sort(out.diff_tab.begin() + t0, out.diff_tab.end());
      for (size_t j = (size_t)t0; j < out.diff_tab.size(); ++j) { out.diff_tab_ne.push_back(diff_seen[(size_t)out.diff_tab[j]]); diff_seen[(size_t)out.diff_tab[j]] = 0; }
      lr.diff_row = (int32_t)out.diff_tab_off.size() - 1;
      out.diff_tab_off.push_back((int32_t)out.diff_tab.size());
      lr.diff_band = !lr.diff_shift && p.diff_launch_banded(out.diff_tab.data() + t0, (int64_t)out.diff_tab.size() - t0);
      lr.diff_shift_band = lr.diff_shift && p.diff_launch_shift_banded(out.diff_tab.data() + t0, out.diff_tab_ne.data() + t0, (int64_t)out.diff_tab.size() - t0);
    }
    if (!kc_is_shared(lr.kclass)) { out.launches.push_back(lr); continue; }
    // a shared class: one launch per table-set group of the records (classify), each with the list of its distinct tables
    const int64_t n_lr = lr.end - lr.begin;
    bool one_group = true;
    for (int64_t i = lr.begin; i < lr.end && one_group; ++i) one_group = U.sh_group[(size_t)U.rec_upd[(size_t)i]] == U.sh_group[(size_t)U.rec_upd[(size_t)lr.begin]];
    if (!one_group) {                               // records group by group, sequence order inside a group
      std::vector<int64_t> perm((size_t)n_lr);
      std::iota(perm.begin(), perm.end(), lr.begin);
      std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return U.sh_group[(size_t)U.rec_upd[(size_t)x]] < U.sh_group[(size_t)U.rec_upd[(size_t)y]]; });
      std::vector<UpdRec> tr((size_t)n_lr); std::vector<int32_t> tu((size_t)n_lr);
      for (int64_t i = 0; i < n_lr; ++i) { tr[(size_t)i] = out.recs[(size_t)perm[(size_t)i]]; tu[(size_t)i] = U.rec_upd[(size_t)perm[(size_t)i]]; }
      std::copy(tr.begin(), tr.end(), out.recs.begin() + lr.begin);
      std::copy(tu.begin(), tu.end(), U.rec_upd.begin() + lr.begin);
    }
    for (int64_t b0 = lr.begin; b0 < lr.end;) {
      const int32_t grp = U.sh_group[(size_t)U.rec_upd[(size_t)b0]];
      LevelRange sub = lr;
      sub.begin = b0; sub.n_recv = sub.n_send = sub.bytes = 0; sub.n_sh = 0;
      int64_t i = b0;
      for (; i < lr.end && U.sh_group[(size_t)U.rec_upd[(size_t)i]] == grp; ++i) {
        const UpdRec& r = out.recs[(size_t)i];
        sub.n_recv += r.n_recv; sub.n_send += r.n_send; sub.bytes += U.rec_bytes[(size_t)U.rec_upd[(size_t)i]];
        const Op* o = ops.data() + r.op_begin;
        for (int q = 0; q < r.n_recv; ++q) {
          const int32_t t = p.f_table[(size_t)o[q].peer];
          bool have = false;
          for (int j = 0; j < sub.n_sh; ++j) have = have || sub.sh_tab[j] == t;
          if (have) continue;
          if (sub.n_sh == SHARED_MAX_TABLES) fail("internal: a launch of a shared class references more tables than its LDS budget holds");
          sub.sh_tab[sub.n_sh++] = t;
        }
      }
      sub.end = i;
      out.launches.push_back(sub);
      b0 = i;
    }
  }
}

// the records of the launch that starts at `begin` in the order perm lists them (indices into out.recs), rec_upd alike
void permute_launch(Schedule& out, std::vector<int32_t>& rec_upd, int64_t begin, const std::vector<int64_t>& perm) {
  std::vector<UpdRec> tr(perm.size()); std::vector<int32_t> tu(perm.size());
  for (size_t i = 0; i < perm.size(); ++i) { tr[i] = out.recs[perm[i]]; tu[i] = rec_upd[perm[i]]; }
  std::copy(tr.begin(), tr.end(), out.recs.begin() + begin);
  std::copy(tu.begin(), tu.end(), rec_upd.begin() + begin);
}

// Inside a launch the order of the records is free (they are independent).  They were placed in SEQUENCE order; what the
// kernels and the Infinity-Cache ticket orders want is MEMORY order — duals and tables lie in factor insertion order — so that
// blocks that are near in the list touch tables that are near in HBM, in every step alike.  The two agree for a sweep in
// insertion order; a backward sweep whose order is the exact reverse of the forward one (a chain of relations through all
// factors: lpmp_plan_suggest_order's answer) lists every level backwards, and a band order across its steps would need block 0
// of one step to wait for the last block of the step before (measured: 6.75 instead of 5.25 ms per pass on the headline grid).
// Records of a launch that are not ascending in the factor index are put in that order (reversed when exactly descending).
void memory_order(Schedule& out, std::vector<int32_t>& rec_upd) {
  for (const auto& lr : out.launches) {
    const int64_t nrec = lr.end - lr.begin;
    if (nrec < 2) continue;
    bool asc = true, desc = true;
    for (int64_t i = lr.begin + 1; i < lr.end && (asc || desc); ++i) {
      asc = asc && out.recs[i - 1].factor <= out.recs[i].factor;
      desc = desc && out.recs[i - 1].factor >= out.recs[i].factor;
    }
    if (asc) continue;
    if (desc) {
      std::reverse(out.recs.begin() + lr.begin, out.recs.begin() + lr.end);
      std::reverse(rec_upd.begin() + lr.begin, rec_upd.begin() + lr.end);
      continue;
    }
    std::vector<int64_t> perm((size_t)nrec);
    std::iota(perm.begin(), perm.end(), lr.begin);
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return out.recs[x].factor < out.recs[y].factor; });
    permute_launch(out, rec_upd, lr.begin, perm);
  }
}

// inside a launch the order of the records is free (they are independent): sub-wave kernels run several
// factors per wavefront, so neighbours in the list should have similar amounts of work.  Sorted inside windows of
// 1024 records only: the order of the sequence carries the model's locality (rows of a grid), and the Infinity-Cache
// ticket orders (chain_plan.cpp, engine.cpp rotation_chain) need blocks that are near in the list to be near in
// the model — sorted globally, the border rows of a grid ended up in the last blocks and no band order was valid
void work_sort(Schedule& out, std::vector<int32_t>& rec_upd) {
  constexpr int64_t SORT_WINDOW = 1024;
  for (const auto& lr : out.launches)
    if (lr.kclass != KC_GENERIC && lr.kclass != KC_DENSE_32 && lr.kclass != KC_DENSE_V32 && lr.kclass != KC_DENSE_BIG && lr.kclass != KC_PW_32 && lr.kclass != KC_SHARED_32 && lr.kclass != KC_DIFF) {   // incl. KC_SMALL
      std::vector<int64_t> perm(lr.end - lr.begin);
      std::iota(perm.begin(), perm.end(), lr.begin);
      // (a launch with many different amounts of work per record — a random graph, degrees 2 ... 25 — has no locality
      // worth keeping and balances better sorted as a whole: C4 12.1 against 13.6 ms per pass)
      std::vector<int32_t> shapes;
      for (int64_t i = lr.begin; i < lr.end && shapes.size() <= 6; ++i) {
        const int32_t sh = out.recs[i].n_recv * 65536 + out.recs[i].n_send;
        if (std::find(shapes.begin(), shapes.end(), sh) == shapes.end()) shapes.push_back(sh);
      }
      const int64_t window = shapes.size() <= 6 ? SORT_WINDOW : std::numeric_limits<int64_t>::max();
      std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) {
        const UpdRec& a = out.recs[x]; const UpdRec& b = out.recs[y];
        const int64_t wx = (x - lr.begin) / window, wy = (y - lr.begin) / window;
        if (wx != wy) return wx < wy;
        return a.n_recv != b.n_recv ? a.n_recv > b.n_recv : a.n_send > b.n_send;
      });
      permute_launch(out, rec_upd, lr.begin, perm);
    }
}

// flags of the fast-class records, kept in recs / ops themselves (packets are plain copies), and the packet stride of every
// launch.  Returns the packet slots of all packed launches.
int64_t packet_flags(Schedule& out) {
  static_assert(sizeof(UpdRec) == sizeof(Op), "a packet slot holds either record");
  int64_t pk_total = 0;                      // (the array is allocated once, by fill_packets)
  for (auto& lr : out.launches) {
    if (kc_is_pw(lr.kclass)) {               // updated pairwise factors: plain packets (no preload / forwarding flags)
      int kmax = 0;
      for (int64_t i = lr.begin; i < lr.end; ++i) kmax = std::max<int>(kmax, out.recs[i].n_recv + out.recs[i].n_send);
      lr.stride = 1 + kmax;
      lr.pk_begin = pk_total;
      pk_total += (lr.end - lr.begin) * lr.stride;
      continue;
    }
    if (lr.kclass == KC_SMALL) {
      for (int64_t i = lr.begin; i < lr.end; ++i) {
        const UpdRec& r = out.recs[i];
        // a send into the peer ONE receive of the record has just rewritten (labeling lists: the middle variables of a
        // triplet): the level loop's staged body (kernels.hip, label_ops_body_staged) hands the rewritten costs over in
        // LDS — receive: pad = 1 (no store), send: pad = index of that receive + 1.  Only a hint: the op-by-op bodies
        // store and reload.
        Op* ow = out.ops.data() + r.op_begin;
        for (int b = r.n_recv; b < r.n_recv + r.n_send; ++b) {
          int hit = -1, n_hit = 0, n_same = 0;
          for (int a = 0; a < r.n_recv; ++a) if (ow[a].peer_dual == ow[b].peer_dual) { hit = a; ++n_hit; }
          for (int b2 = r.n_recv; b2 < r.n_recv + r.n_send; ++b2) if (ow[b2].peer_dual == ow[b].peer_dual) ++n_same;
          if (n_hit == 1 && n_same == 1 && hit < 8 && ow[hit].peer_const == ow[b].peer_const && ow[hit].pd0 == ow[b].pd0 && ow[hit].pd1 == ow[b].pd1) { ow[hit].pad = 1; ow[b].pad = hit + 1; }
        }
      }
      continue;
    }
    if (!kc_is_packed(lr.kclass) && !kc_is_shared(lr.kclass)) continue;   // (shared classes: packets / indirect records as the packed classes)
    if (kc_is_var(lr.kclass)) {
      // the padded classes only exist in packed / indirect form: a launch with a record of more ops than the slab holds goes to
      // the streaming kernel, which works op by op.  (Records with duplicate vectors are not among them: cls_of already gave
      // them an op-by-op class.)
      bool ok = true;
      for (int64_t i = lr.begin; i < lr.end && ok; ++i) if (out.recs[i].n_recv + out.recs[i].n_send > pk_class_cap(lr.kclass)) ok = false;
      if (!ok) { lr.kclass = KC_DENSE_BIG; continue; }
    }
    // flags of the records (independent of each other: chunks of the launch on several threads), then the packet stride
    const int64_t n_lr = lr.end - lr.begin;
    std::vector<int> kmax_of(PLAN_MAX_THREADS, 0);
    parallel_chunks(n_lr, 32768, [&](int64_t c0, int64_t c1, int thread) {
      int kmax_l = 0;
      for (int64_t i = lr.begin + c0; i < lr.begin + c1; ++i) {
        UpdRec& r = out.recs[i];
        Op* o = out.ops.data() + r.op_begin;
        kmax_l = std::max<int>(kmax_l, r.n_recv + r.n_send);
        bool preload_ok = true;   // a send may be requested early unless a receive of this update writes the same vector
        for (int a = 0; a < r.n_recv && preload_ok; ++a)
          for (int b = r.n_recv; b < r.n_recv + r.n_send; ++b)
            if (same_vector(o[a], o[b])) { preload_ok = false; break; }
        if (preload_ok) r.kind_flags |= UPD_PRELOAD_OK;
        // register forwarding: send b targets the vector receive a (one of the first 4) has just rewritten ->
        // the receive keeps its result in a register (pad = 1: no store) and the send reads it from there
        // (pad = a + 1); at most one send per receive, and only if no other receive/send touches that vector
        for (int b = r.n_recv; b < r.n_recv + r.n_send && b - r.n_recv < 4; ++b) {
          int hit = -1, n_hit = 0, n_send_same = 0;
          for (int a = 0; a < r.n_recv; ++a) if (same_vector(o[a], o[b])) { hit = a; ++n_hit; }
          for (int b2 = r.n_recv; b2 < r.n_recv + r.n_send; ++b2) if (same_vector(o[b2], o[b])) ++n_send_same;
          if (n_hit == 1 && n_send_same == 1 && hit < 4) { o[hit].pad = 1; o[b].pad = hit + 1; }
        }
      }
      kmax_of[(size_t)thread] = kmax_l;
    });
    const int kmax = *std::max_element(kmax_of.begin(), kmax_of.end());
    // (records with duplicate messages or more ops than the LDS slab holds never get here: cls_of gives them an op-by-op class)
    if (kmax > pk_class_cap(lr.kclass)) fail("internal: a record of a packed class has more ops than its LDS slab holds");
    if (kmax > PK_MAX_OPS) {                 // too many ops for a packet: indirect mode
      lr.stride = -1;
      continue;
    }
    lr.stride = 1 + kmax;
    lr.pk_begin = pk_total;                  // (filled by fill_packets, when the size of the whole array is known)
    pk_total += n_lr * lr.stride;
  }
  return pk_total;
}

// packets: ONE allocation, never zero-filled (every slot is written: the record, its ops, zeros behind them)
void fill_packets(Schedule& out, int64_t pk_total) {
  out.packets.resize((size_t)pk_total);
  for (const auto& lr : out.launches) {
    if (lr.stride <= 0) continue;
    parallel_chunks(lr.end - lr.begin, 32768, [&](int64_t c0, int64_t c1, int) {
      for (int64_t i = lr.begin + c0; i < lr.begin + c1; ++i) {
        Op* slot = out.packets.data() + lr.pk_begin + (i - lr.begin) * lr.stride;
        const UpdRec& r = out.recs[i];
        std::memcpy(slot, &r, sizeof(Op));
        const int n = r.n_recv + r.n_send;
        for (int k = 0; k < n; ++k) slot[1 + k] = out.ops[r.op_begin + k];
        if (n + 1 < lr.stride) std::memset((void*)(slot + 1 + n), 0, (size_t)(lr.stride - 1 - n) * sizeof(Op));
      }
    });
  }
}

}  // namespace

void Plan::make_schedule(const std::vector<Segment>& segs, bool fuse, Schedule& out, bool chains, std::vector<int32_t>* levels_only) const {
  out = Schedule();
  const bool timed_ = std::getenv("LPMP_PLAN_TIMES") != nullptr;
  auto t_last_ = std::chrono::steady_clock::now();
  auto lap_ = [&](const char* what) { if (!timed_) return; const auto now = std::chrono::steady_clock::now(); std::fprintf(stderr, "lpmp: make_schedule %-8s %.0f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last_).count()); t_last_ = now; };
  Updates U;
  gather_rows(*this, segs, U);
  lap_("rows");
  level_recurrence(*this, fuse, U);
  lap_("levels");
  out.n_levels = U.max_level;
  if (levels_only) {
    levels_only->resize((size_t)U.N);
    for (int64_t u = 0; u < U.N; ++u) {
      const int32_t o = U.owner[u];
      (*levels_only)[(size_t)u] = (U.n_recv_of[o] + U.n_send_of[o] > 0 || ftype_primal[f_type[U.uf[o]]]) ? U.level[o] : 0;
    }
    return;
  }
  OpVec ops;
  out.alg_bytes = build_ops(*this, U, ops);
  lap_("ops");
  classify(*this, U, ops);
  lap_("dup");
  bucket(*this, U, ops, out);
  memory_order(out, U.rec_upd);
  lap_("records");
  out.ops = std::move(ops);
  work_sort(out, U.rec_upd);
  lap_("sorted");
  const int64_t pk_total = packet_flags(out);
  lap_("pk-flags");
  fill_packets(out, pk_total);
  lap_("packets");
  if (!chains && U.max_level == 3) return;
  plan_chains(*this, UpdateView{U.N, U.uf.data(), U.owner.data(), U.uom.data(), U.umk.data()}, U.rec_upd, chain_settings_from_env(), out);
}


// reference factors_messages.hxx:2699-2744.  A dispatcher = the run of list entries with one message type and role; a
// batch-capable one (MessageDispatcher::CanCallSendMessages: SendMessagesToRight for left-role entries, ...ToLeft for
// right-role ones) with MORE THAN ONE active message (omega > 0) makes one call with the sum of the run's weights;
// the device batch op (lpmp_msg_flags) gives each active message sum / n_active times the plain message.
void Plan::effective_send_weights(int32_t f, const double* omega, double* w) const {
  int64_t k = 0;
  for (int64_t j = fm_off[f]; j < fm_off[f + 1];) {
    int64_t j2 = j;
    while (j2 < fm_off[f + 1] && m_type[fm[j2].msg] == m_type[fm[j].msg] && fm[j2].role == fm[j].role) ++j2;
    if (!fm[j].sends) { j = j2; continue; }
    const int64_t n = j2 - j;
    const int fl = mtypes[m_type[fm[j].msg]].flags;
    const bool batch = fm[j].role == 0 ? (fl & LPMP_MF_BATCH_TO_RIGHT) != 0 : (fl & LPMP_MF_BATCH_TO_LEFT) != 0;
    if (batch) {
      int64_t n_active = 0; double sum = 0.0;
      for (int64_t i = 0; i < n; ++i) { if (omega[k + i] > 0.0) ++n_active; sum += omega[k + i]; }
      const double each = n_active > 1 ? sum / double(n_active) : 0.0;
      for (int64_t i = 0; i < n; ++i) w[k + i] = omega[k + i] > 0.0 ? (n_active > 1 ? each : omega[k + i]) : 0.0;
    } else {
      for (int64_t i = 0; i < n; ++i) w[k + i] = omega[k + i];
    }
    k += n; j = j2;
  }
}

// send_messages_with_adaptive_weights (reference factors_messages.hxx:2860-2926) walks ALL dispatchers of the factor
// with the iterator over the SENDING weights: defined only when every message of an updated factor sends; its batch
// branch (and send_messages_residual's) calls op members no device op is defined for
std::string Plan::adaptive_obstacle() const {
  if (any_batch) return "adaptive sends with batch-capable message ops are not built";
  for (int64_t f = 0; f < nf; ++f) {
    if (!updated[f]) continue;
    bool any = false, all = true;
    for (int64_t j = fm_off[f]; j < fm_off[f + 1]; ++j) { any = any || fm[j].sends; all = all && fm[j].sends; }
    if (any && !all) return "adaptive sends: factor " + std::to_string(f) + " has messages it does not send through (undefined in the reference)";
  }
  return "";
}

// ---- conditional rounding from the duals (plan.hpp, DecodePlan) ---------------------------------------------------------
DecodePlan Plan::decode_plan(int direction) const {
  DecodePlan dp;
  if (direction < 0 || direction > 1) fail("decode plan: bad direction");
  // the refusals: the lowest factor that breaks the rule of the supported models, and what it breaks
  int64_t bad = nf; const char* what = "";
  auto offend = [&](int64_t f, const char* w) { if (f < bad) { bad = f; what = w; } };
  std::vector<int32_t> side_unary(2 * (size_t)nf, -1);       // [pairwise factor][side]: the unary of that side
  std::vector<uint8_t> side_count(2 * (size_t)nf, 0);
  for (int64_t m = 0; m < nm; ++m) {
    const int32_t l = m_left[m], r = m_right[m];
    if (mtypes[m_type[m]].kind != LPMP_M_UNARY_PAIRWISE) { offend(std::min(l, r), "has a message that is not a unary-pairwise one"); continue; }
    const size_t slot = 2 * (size_t)r + mtypes[m_type[m]].param;
    if (side_count[slot] < 2) ++side_count[slot];
    side_unary[slot] = l;
  }
  for (int64_t f = 0; f < nf && f < bad; ++f) {
    if (f_kind[f] == LPMP_F_VECTOR) continue;
    const size_t s = 2 * (size_t)f;
    if (side_count[s] == 0 || side_count[s + 1] == 0) offend(f, "is a pairwise factor with a side that has no unary");
    else if (side_count[s] > 1 || side_count[s + 1] > 1) offend(f, "is a pairwise factor with two unaries on one side");
    else if (side_unary[s] == side_unary[s + 1]) offend(f, "is a pairwise factor with one unary on both sides");
  }
  if (bad < nf) {
    dp.bad_factor = (int32_t)bad;
    dp.why = "decode: factor " + std::to_string(bad) + " " + what + " (DESIGN.md 8)";
    return dp;
  }
  // pi, positions, edges in ascending message index
  std::vector<int32_t> pos((size_t)nf, -1);
  for (int32_t f : order[direction]) if (f_kind[f] == LPMP_F_VECTOR) { pos[(size_t)f] = (int32_t)dp.unaries.size(); dp.unaries.push_back(f); }
  const size_t nu = dp.unaries.size();
  dp.edge_off.assign(nu + 1, 0);
  for (int64_t m = 0; m < nm; ++m) ++dp.edge_off[(size_t)pos[(size_t)m_left[m]] + 1];
  std::partial_sum(dp.edge_off.begin(), dp.edge_off.end(), dp.edge_off.begin());
  dp.edges.resize((size_t)nm);
  {
    std::vector<int64_t> cur(dp.edge_off.begin(), dp.edge_off.end() - 1);
    for (int64_t m = 0; m < nm; ++m) {
      const int32_t r = m_right[m], side = mtypes[m_type[m]].param;
      dp.edges[(size_t)cur[(size_t)pos[(size_t)m_left[m]]]++] = {r, side, side_unary[2 * (size_t)r + (1 - side)]};
    }
  }
  dp.level.assign(nu, 1);
  for (size_t i = 0; i < nu; ++i) {
    int32_t lv = 1;
    for (int64_t k = dp.edge_off[i]; k < dp.edge_off[i + 1]; ++k) {
      const size_t j = (size_t)pos[(size_t)dp.edges[(size_t)k].other];
      if (j < i) lv = std::max(lv, dp.level[j] + 1);
    }
    dp.level[i] = lv;
    dp.n_levels = std::max(dp.n_levels, lv);
  }
  return dp;
}

// ---- what path moves and forest moves take (plan.hpp, PairSides) ----------------------------------------------------------------
static bool is_unary_pairwise(const Plan& p, int64_t m) {
  const lpmp_msg_type& mt = p.mtypes[(size_t)p.m_type[(size_t)m]];
  return mt.kind == LPMP_M_UNARY_PAIRWISE && (mt.param == 0 || mt.param == 1) && p.f_kind[p.m_left[(size_t)m]] == LPMP_F_VECTOR &&
         p.f_kind[p.m_right[(size_t)m]] != LPMP_F_VECTOR;
}
PairSides Plan::pair_sides() const {
  PairSides ps;
  ps.side_unary.assign(2 * (size_t)nf, -1);
  ps.side_count.assign(2 * (size_t)nf, 0);
  for (int64_t m = 0; m < nm; ++m) {
    if (!is_unary_pairwise(*this, m)) continue;
    const size_t slot = 2 * (size_t)m_right[(size_t)m] + (size_t)mtypes[(size_t)m_type[(size_t)m]].param;
    if (ps.side_count[slot] < 2) ++ps.side_count[slot];
    ps.side_unary[slot] = m_left[(size_t)m];
  }
  return ps;
}
std::string Plan::move_obstacle(int32_t u, const PairSides& ps, const char* move) const {
  auto S = [](int64_t v) { return std::to_string(v); };
  if (f_dim0[u] > PATH_MAX_LABELS) return "has " + S(f_dim0[u]) + " labels (a " + move + " move takes at most " + S(PATH_MAX_LABELS) + ")";
  for (int64_t k = fm_off[(size_t)u]; k < fm_off[(size_t)u + 1]; ++k) {
    const MsgEntry& me = fm[(size_t)k];
    if (me.role != 0 || !is_unary_pairwise(*this, me.msg)) return "has a message that is not a unary-pairwise message with the factor as its unary";
    const size_t s = 2 * (size_t)m_right[(size_t)me.msg];
    if (ps.side_count[s] != 1 || ps.side_count[s + 1] != 1 || ps.side_unary[s] == ps.side_unary[s + 1])
      return "is next to pairwise factor " + S(m_right[(size_t)me.msg]) + ", which does not have exactly one unary on each side from two different unaries";
  }
  return "";
}

// ---- the stages path_plan and forest_plan share ---------------------------------------------------------------------------------
namespace {
std::string S(int64_t v) { return std::to_string(v); }
// group_off [n_groups + 1] starts at 0 and never decreases
void check_group_off(int64_t n_groups, const int64_t* group_off, const std::string& who) {
  if (group_off[0] != 0) fail(who + ": group_off[0] is " + S(group_off[0]) + ", not 0");
  for (int64_t g = 0; g < n_groups; ++g)
    if (group_off[g + 1] < group_off[g]) fail(who + ": group_off is not monotone at group " + S(g));
}
// the ne listed members, group g holding the entries [first(g), first(g + 1)): every one a VECTOR factor of the plan, none twice
// in its group.  grp_of / ent_of [nf] are the scan's stamps (the group a factor was last seen in, and its entry there)
template <class First>
void check_members(const Plan& p, int64_t ne, const int32_t* un, int64_t n_groups, First first, const std::string& who,
                   std::vector<int64_t>& grp_of, std::vector<int64_t>& ent_of) {
  for (int64_t e = 0; e < ne; ++e) {
    const int32_t f = un[e];
    if (f < 0 || f >= p.nf) fail(who + ": factor index " + S(f) + " (entry " + S(e) + ") is out of range");
    if (p.f_kind[f] != LPMP_F_VECTOR) fail(who + ": factor " + S(f) + " (entry " + S(e) + ") is not a VECTOR factor");
  }
  grp_of.assign((size_t)p.nf, -1); ent_of.assign((size_t)p.nf, 0);
  for (int64_t g = 0; g < n_groups; ++g)
    for (int64_t e = first(g); e < first(g + 1); ++e) {
      const size_t f = (size_t)un[e];
      if (grp_of[f] == g) fail(who + ": factor " + S(un[e]) + " (entry " + S(e) + ") appears twice in group " + S(g) + " (first: entry " + S(ent_of[f]) + ")");
      grp_of[f] = g; ent_of[f] = e;
    }
}
// the unsupported shapes: the lowest listed unary that has one goes into `bad`, and the text of `why` comes back ("": none has)
std::string lowest_obstacle(const Plan& p, int64_t ne, const int32_t* un, const PairSides& sides, const char* move, const std::string& who, int32_t& bad) {
  std::string what;
  for (int64_t e = 0; e < ne; ++e) {
    const int32_t u = un[e];
    if (bad >= 0 && u >= bad) continue;
    const std::string w = p.move_obstacle(u, sides, move);
    if (!w.empty()) { bad = u; what = w; }
  }
  return bad < 0 ? "" : who + ": factor " + S(bad) + " " + what + " (DESIGN.md 8, " + move + " moves)";
}
// the messages of unary u in ascending message index: the order of its links
void sorted_messages(const Plan& p, int32_t u, std::vector<int32_t>& msgs) {
  msgs.clear();
  for (int64_t k = p.fm_off[(size_t)u]; k < p.fm_off[(size_t)u + 1]; ++k) msgs.push_back(p.fm[(size_t)k].msg);
  std::sort(msgs.begin(), msgs.end());
}
}  // namespace

// ---- path moves (plan.hpp, PathPlan) ----------------------------------------------------------------------------------------
PathPlan Plan::path_plan(int64_t n_groups, const int64_t* group_off, const int64_t* path_off, const int32_t* un, const std::string& who) const {
  PathPlan pp;
  if (n_groups < 0 || !group_off || !path_off) fail(who + ": bad argument");
  check_group_off(n_groups, group_off, who);
  const int64_t n_paths = group_off[n_groups];
  if (path_off[0] != 0) fail(who + ": path_off[0] is " + S(path_off[0]) + ", not 0");
  for (int64_t j = 0; j < n_paths; ++j)
    if (path_off[j + 1] <= path_off[j]) fail(who + ": path_off is not increasing at path " + S(j) + " (a path has at least one member)");
  const int64_t ne = path_off[n_paths];
  if (ne > (int64_t)std::numeric_limits<int32_t>::max()) fail(who + ": more than 2^31 entries");
  if (ne > 0 && !un) fail(who + ": null list of unaries");
  // where a unary sits in the group at hand: group stamp, path, index in the path, entry
  std::vector<int64_t> grp_of, path_of((size_t)nf, 0), ent_of;
  check_members(*this, ne, un, n_groups, [&](int64_t g) { return path_off[group_off[g]]; }, who, grp_of, ent_of);
  pp.group_off.assign(group_off, group_off + n_groups + 1);
  pp.path_off.assign(path_off, path_off + n_paths + 1);
  pp.unaries.assign(un, un + ne);
  // the unary on each side of every pairwise factor, from all unary-pairwise messages (as in decode_plan)
  const PairSides sides = pair_sides();
  const std::vector<int32_t>& side_unary = sides.side_unary;
  pp.why = lowest_obstacle(*this, ne, un, sides, "path", who, pp.bad_factor);
  if (!pp.why.empty()) return pp;
  // links in ascending message index, and the path edges
  pp.edge.assign((size_t)ne, -1); pp.edge_prev_side.assign((size_t)ne, 0);
  pp.link_off.assign(1, 0);
  std::fill(grp_of.begin(), grp_of.end(), -1);
  std::vector<int32_t> msgs;
  for (int64_t g = 0; g < n_groups; ++g) {
    for (int64_t j = group_off[g]; j < group_off[g + 1]; ++j)
      for (int64_t e = path_off[j]; e < path_off[j + 1]; ++e) { const size_t f = (size_t)un[e]; grp_of[f] = g; path_of[f] = j; ent_of[f] = e; }
    for (int64_t j = group_off[g]; j < group_off[g + 1]; ++j) {
      pp.longest = std::max(pp.longest, path_off[j + 1] - path_off[j]);
      for (int64_t e = path_off[j]; e < path_off[j + 1]; ++e) {
        const int32_t u = un[e];
        pp.max_labels = std::max(pp.max_labels, f_dim0[u]);
        sorted_messages(*this, u, msgs);
        for (int32_t m : msgs) {
          const int32_t p = m_right[(size_t)m], side = mtypes[(size_t)m_type[(size_t)m]].param, v = side_unary[2 * (size_t)p + (size_t)(1 - side)];
          int32_t on_path = 0;
          if (grp_of[(size_t)v] == g) {
            const std::string pair = "pairwise factor " + S(p) + " joins factor " + S(u) + " (entry " + S(e) + ") and factor " + S(v) + " (entry " + S(ent_of[(size_t)v]) + ")";
            if (path_of[(size_t)v] != j) fail(who + ": " + pair + ", members of two paths of group " + S(g));
            const int64_t di = ent_of[(size_t)v] - e;
            if (di != 1 && di != -1) fail(who + ": " + pair + ", two non-consecutive members of path " + S(j) + " (a closed ring included)");
            if (di == -1) {
              if (pp.edge[(size_t)e] >= 0)
                fail(who + ": more than one pairwise factor (" + S(pp.edge[(size_t)e]) + " and " + S(p) + ") joins factor " + S(v) + " (entry " + S(e - 1) + ") and factor " + S(u) + " (entry " + S(e) + ")");
              pp.edge[(size_t)e] = p; pp.edge_prev_side[(size_t)e] = 1 - side;
            }
            on_path = 1;
          }
          pp.links.push_back({p, side, v, on_path});
          if (!on_path) ++pp.n_off_path_links;
        }
        pp.link_off.push_back((int64_t)pp.links.size());
        if (e > path_off[j] && pp.edge[(size_t)e] < 0)
          fail(who + ": no pairwise factor joins factor " + S(un[e - 1]) + " (entry " + S(e - 1) + ") and factor " + S(u) + " (entry " + S(e) + ")");
      }
      pp.n_path_edges += path_off[j + 1] - path_off[j] - 1;
    }
  }
  if (pp.links.size() > (size_t)std::numeric_limits<int32_t>::max()) fail(who + ": more than 2^31 links");
  return pp;
}

// ---- forest moves (plan.hpp, ForestPlan) --------------------------------------------------------------------------------------
ForestPlan Plan::forest_plan(int64_t n_groups, const int64_t* group_off, const int32_t* un, const int32_t* par, const std::string& who) const {
  ForestPlan fp;
  if (n_groups < 0 || !group_off) fail(who + ": bad argument");
  check_group_off(n_groups, group_off, who);
  const int64_t ne = group_off[n_groups];
  if (ne > (int64_t)std::numeric_limits<int32_t>::max()) fail(who + ": more than 2^31 entries");
  if (ne > 0 && (!un || !par)) fail(who + ": null list of unaries or parents");
  // where a unary sits in the group at hand: group stamp and entry
  std::vector<int64_t> grp_of, ent_of;
  check_members(*this, ne, un, n_groups, [&](int64_t g) { return group_off[g]; }, who, grp_of, ent_of);
  fp.group_off.assign(group_off, group_off + n_groups + 1);
  fp.unaries.assign(un, un + ne);
  fp.parent.assign(par, par + ne);
  fp.parent_entry.assign((size_t)ne, -1);
  std::fill(grp_of.begin(), grp_of.end(), -1);
  for (int64_t g = 0; g < n_groups; ++g) {
    for (int64_t e = group_off[g]; e < group_off[g + 1]; ++e) { grp_of[(size_t)un[e]] = g; ent_of[(size_t)un[e]] = e; }
    for (int64_t e = group_off[g]; e < group_off[g + 1]; ++e) {
      const int32_t q = par[e];
      if (q == -1) continue;
      if (q == un[e]) fail(who + ": factor " + S(un[e]) + " (entry " + S(e) + ") is its own parent");
      if (q < 0 || q >= nf || grp_of[(size_t)q] != g)
        fail(who + ": the parent " + S(q) + " of factor " + S(un[e]) + " (entry " + S(e) + ") is neither -1 nor a member of group " + S(g));
      fp.parent_entry[(size_t)e] = (int32_t)ent_of[(size_t)q];
    }
  }
  // cycles of parent pointers: walk up from every entry; a walk that meets itself has found one.  The lowest entry on any
  { std::vector<int64_t> seen((size_t)ne, -1);      // the walk that reached the entry
    int64_t lowest = -1;
    for (int64_t e0 = 0; e0 < ne; ++e0) {
      int64_t e = e0;
      while (e >= 0 && seen[(size_t)e] < 0) { seen[(size_t)e] = e0; e = fp.parent_entry[(size_t)e]; }
      if (e < 0 || seen[(size_t)e] != e0) continue;
      int64_t lo = e;
      for (int64_t c = fp.parent_entry[(size_t)e]; c != e; c = fp.parent_entry[(size_t)c]) lo = std::min(lo, c);
      if (lowest < 0 || lo < lowest) lowest = lo;
    }
    if (lowest >= 0) fail(who + ": the parent pointers close a cycle through factor " + S(un[lowest]) + " (entry " + S(lowest) + ")");
  }
  const PairSides sides = pair_sides();
  fp.why = lowest_obstacle(*this, ne, un, sides, "forest", who, fp.bad_factor);
  if (!fp.why.empty()) return fp;
  // links in ascending message index, the tree edges and the children
  fp.edge.assign((size_t)ne, -1); fp.edge_side.assign((size_t)ne, 0);
  fp.link_off.assign(1, 0); fp.child_off.assign(1, 0);
  fp.height.assign((size_t)ne, 0); fp.depth.assign((size_t)ne, -1);
  fp.group_height.assign((size_t)n_groups, -1);
  std::fill(grp_of.begin(), grp_of.end(), -1);
  std::vector<int32_t> msgs, by_depth;
  for (int64_t g = 0; g < n_groups; ++g) {
    const int64_t b = group_off[g], en = group_off[g + 1];
    for (int64_t e = b; e < en; ++e) { grp_of[(size_t)un[e]] = g; ent_of[(size_t)un[e]] = e; }
    for (int64_t e = b; e < en; ++e) {
      const int32_t u = un[e];
      fp.max_labels = std::max(fp.max_labels, f_dim0[u]);
      sorted_messages(*this, u, msgs);
      for (int32_t m : msgs) {
        const int32_t p = m_right[(size_t)m], side = mtypes[(size_t)m_type[(size_t)m]].param, v = sides.side_unary[2 * (size_t)p + (size_t)(1 - side)];
        int32_t tree = 0;
        if (grp_of[(size_t)v] == g) {
          const int64_t ev = ent_of[(size_t)v];
          if (fp.parent_entry[(size_t)e] == ev) {
            if (fp.edge[(size_t)e] >= 0)
              fail(who + ": more than one pairwise factor (" + S(fp.edge[(size_t)e]) + " and " + S(p) + ") joins factor " + S(u) + " (entry " + S(e) + ") and its parent, factor " + S(v) + " (entry " + S(ev) + ")");
            fp.edge[(size_t)e] = p; fp.edge_side[(size_t)e] = side;
            tree = 1;
          } else if (fp.parent_entry[(size_t)ev] == e) {
            fp.children.push_back((int32_t)ev);     // (a second factor to the same child: refused at the child)
            tree = 2;
          } else {
            fail(who + ": pairwise factor " + S(p) + " joins factor " + S(u) + " (entry " + S(e) + ") and factor " + S(v) + " (entry " + S(ev) + "), members of group " + S(g) +
                 " that are not child and parent (the members of a group must induce a forest)");
          }
        }
        fp.links.push_back({p, side, v, tree});
        if (!tree) ++fp.n_off_tree_links;
      }
      fp.link_off.push_back((int64_t)fp.links.size());
      fp.child_off.push_back((int64_t)fp.children.size());
      if (fp.parent_entry[(size_t)e] >= 0) {
        if (fp.edge[(size_t)e] < 0)
          fail(who + ": no pairwise factor joins factor " + S(u) + " (entry " + S(e) + ") and its parent, factor " + S(par[e]) + " (entry " + S(fp.parent_entry[(size_t)e]) + ")");
        ++fp.n_tree_edges;
      } else ++fp.n_trees;
    }
    // depths (walk up to the first entry that has one), then heights from the deepest entries upwards
    for (int64_t e0 = b; e0 < en; ++e0) {
      int32_t steps = 0;
      int64_t e = e0;
      while (fp.depth[(size_t)e] < 0 && fp.parent_entry[(size_t)e] >= 0) { e = fp.parent_entry[(size_t)e]; ++steps; }
      int32_t d = (fp.depth[(size_t)e] < 0 ? 0 : fp.depth[(size_t)e]) + steps;
      for (e = e0; fp.depth[(size_t)e] < 0; e = fp.parent_entry[(size_t)e]) { fp.depth[(size_t)e] = d--; if (fp.parent_entry[(size_t)e] < 0) break; }
    }
    by_depth.clear();
    for (int64_t e = b; e < en; ++e) by_depth.push_back((int32_t)e);
    std::stable_sort(by_depth.begin(), by_depth.end(), [&](int32_t x, int32_t y) { return fp.depth[(size_t)x] > fp.depth[(size_t)y]; });
    for (int32_t e : by_depth) {
      const int32_t q = fp.parent_entry[(size_t)e];
      if (q >= 0) fp.height[(size_t)q] = std::max(fp.height[(size_t)q], fp.height[(size_t)e] + 1);
      fp.group_height[(size_t)g] = std::max(fp.group_height[(size_t)g], fp.height[(size_t)e]);
    }
    fp.max_height = std::max(fp.max_height, fp.group_height[(size_t)g]);
  }
  if (fp.links.size() > (size_t)std::numeric_limits<int32_t>::max()) fail(who + ": more than 2^31 links");
  return fp;
}

// ---- moving label windows (plan.hpp, WindowPlan) ----------------------------------------------------------------------------------
WindowPlan Plan::window_plan(int64_t n, const int32_t* factors, const std::string& who) const {
  WindowPlan w;
  const Plan& p = *this;
  std::vector<int32_t> row_of((size_t)p.nf, -1);
  if (!factors) { for (int64_t f = 0; f < p.nf; ++f) if (p.f_kind[f] == LPMP_F_VECTOR) { row_of[(size_t)f] = (int32_t)w.factors.size(); w.factors.push_back((int32_t)f); } }
  else {
    if (n > (int64_t)std::numeric_limits<int32_t>::max()) fail(who + ": more than 2^31 factors listed");
    w.factors.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      const int32_t f = factors[i];
      if (f < 0 || f >= p.nf) fail(who + ": factor index " + std::to_string(f) + " (entry " + std::to_string(i) + ") is out of range");
      if (p.f_kind[f] != LPMP_F_VECTOR) fail(who + ": factor " + std::to_string(f) + " (entry " + std::to_string(i) + ") is not a VECTOR factor");
      if (row_of[(size_t)f] >= 0) fail(who + ": factor " + std::to_string(f) + " (entry " + std::to_string(i) + ") is listed twice");
      row_of[(size_t)f] = (int32_t)i;
      w.factors.push_back(f);
    }
  }
  int32_t bad = -1; std::string why;
  auto refuse = [&](int32_t u, const std::string& what) { if (bad < 0 || u < bad) { bad = u; why = what; } };
  // the unary on each side of a DIFF_SHIFT factor, from ALL its unary-pairwise messages (-1: none, -2: two different ones)
  auto side_unaries = [&](int32_t pw, int32_t out[2]) {
    out[0] = out[1] = -1;
    for (int64_t k = p.fm_off[(size_t)pw]; k < p.fm_off[(size_t)pw + 1]; ++k) {
      const MsgEntry& me = p.fm[(size_t)k];
      const lpmp_msg_type& mt = p.mtypes[(size_t)p.m_type[(size_t)me.msg]];
      if (me.role != 1 || mt.kind != LPMP_M_UNARY_PAIRWISE || (mt.param != 0 && mt.param != 1)) continue;
      const int32_t u = p.m_left[(size_t)me.msg];
      int32_t& slot = out[mt.param];
      slot = slot == -1 || slot == u ? u : -2;
    }
  };
  std::vector<int32_t> pair_of((size_t)p.nf, -1);
  w.link_off.assign(1, 0);
  for (size_t i = 0; i < w.factors.size(); ++i) {
    const int32_t u = w.factors[i], d = p.f_dim0[u];
    w.max_labels = std::max(w.max_labels, d);
    if (d > MOVE_MAX_LABELS) refuse(u, "has " + std::to_string(d) + " labels (a wave holds a vector of at most " + std::to_string(MOVE_MAX_LABELS) + ")");
    const size_t first = w.links.size();
    for (int64_t k = p.fm_off[(size_t)u]; k < p.fm_off[(size_t)u + 1]; ++k) {
      const MsgEntry& me = p.fm[(size_t)k];
      const lpmp_msg_type& mt = p.mtypes[(size_t)p.m_type[(size_t)me.msg]];
      const int32_t pw = me.role == 0 ? p.m_right[(size_t)me.msg] : -1;
      if (mt.kind != LPMP_M_UNARY_PAIRWISE || pw < 0 || p.f_kind[pw] != LPMP_F_PAIRWISE_DIFF_SHIFT || (mt.param != 0 && mt.param != 1)) {
        refuse(u, "has a message that is not a unary-pairwise message with the factor as its unary and a DIFF_SHIFT factor on the right");
        continue;
      }
      const int32_t side = mt.param;
      if ((side ? p.f_dim1[pw] : p.f_dim0[pw]) != d) { refuse(u, "and side " + std::to_string(side) + " of factor " + std::to_string(pw) + " differ in their label counts"); continue; }
      bool twice = false;
      for (size_t q = first; q < w.links.size(); ++q) twice = twice || (w.links[q].p == pw && w.links[q].side == side);
      if (twice) { refuse(u, "has two messages into one vector of factor " + std::to_string(pw)); continue; }
      w.links.push_back({pw, side});
      if (pair_of[(size_t)pw] < 0) {
        int32_t su[2];
        side_unaries(pw, su);
        if (su[0] == -2 || su[1] == -2) { refuse(u, "is next to DIFF_SHIFT factor " + std::to_string(pw) + ", which has two different unaries on one side"); pair_of[(size_t)pw] = -2; continue; }
        pair_of[(size_t)pw] = (int32_t)w.pairs.size();
        w.pairs.push_back({pw, su[0] >= 0 ? row_of[(size_t)su[0]] : -1, su[1] >= 0 ? row_of[(size_t)su[1]] : -1});
      } else if (pair_of[(size_t)pw] == -2) refuse(u, "is next to DIFF_SHIFT factor " + std::to_string(pw) + ", which has two different unaries on one side");
    }
    w.link_off.push_back((int64_t)w.links.size());
  }
  if (w.links.size() > (size_t)std::numeric_limits<int32_t>::max()) fail(who + ": more than 2^31 links");
  if (bad >= 0) {
    w.bad_factor = bad;
    w.why = who + ": factor " + std::to_string(bad) + " " + why + " (DESIGN.md 4, moving label windows)";
  }
  return w;
}

// ---- partition sweeps (reference LP_MP.h:1717-1843).  union_find.hxx:5-93: union by size, the first argument's root
// wins ties, contiguous ids in increasing root index; partitions without updated factors are dropped (:1736-1745).
// Intra-partition order: the reference sorts by position in forwardOrdering_ with a comparator that is false for every
// pair (`std::get<0>(a) < std::get<0>(a)`, :1775), so the result depends on the standard library's sort; the engine
// keeps the order the partition was populated in (insertion order of the updated factors, :1755-1760) — what a stable
// sort returns for that comparator, and what libstdc++'s std::sort leaves for partitions of up to 16 factors.
void Plan::ensure_partition() {
  if (part.valid) return;
  part = Partition();
  std::vector<int64_t> id(nf), sz(nf, 1);
  std::iota(id.begin(), id.end(), 0);
  auto find = [&](int64_t p) {
    int64_t root = p;
    while (root != id[root]) root = id[root];
    while (p != root) { const int64_t nx = id[p]; id[p] = root; p = nx; }
    return root;
  };
  for (size_t k = 0; k + 1 < part_pairs.size(); k += 2) {
    const int64_t i = find(part_pairs[k]), j = find(part_pairs[k + 1]);
    if (i == j) continue;
    if (sz[i] < sz[j]) { id[i] = j; sz[j] += sz[i]; } else { id[j] = i; sz[i] += sz[j]; }
  }
  std::vector<int64_t> root_id(nf, -1), count;
  for (int64_t i = 0; i < nf; ++i) root_id[find(i)] = 1;
  int64_t next = 0;
  for (int64_t d = 0; d < nf; ++d) if (root_id[d] == 1) root_id[d] = next++;
  count.assign(next, 0);
  for (int64_t i = 0; i < nf; ++i) if (updated[i]) count[root_id[find(i)]]++;
  std::vector<int64_t> part_of(next, -1);
  int64_t P = 0;
  for (int64_t c = 0; c < next; ++c) if (count[c] > 0) part_of[c] = P++;
  if (P == 0) fail("partition sweeps: the model has no updated factor");
  part.off.assign(P + 1, 0);
  for (int64_t c = 0; c < next; ++c) if (part_of[c] >= 0) part.off[part_of[c] + 1] = count[c];
  std::partial_sum(part.off.begin(), part.off.end(), part.off.begin());
  part.f.resize(part.off[P]);
  {
    std::vector<int64_t> cur(part.off.begin(), part.off.end() - 1);
    for (int64_t i = 0; i < nf; ++i) if (updated[i]) part.f[cur[part_of[root_id[find(i)]]]++] = (int32_t)i;
  }
  auto seg = [&](int64_t a, bool rev_a, int64_t b, bool rev_b) {
    SegList s;
    auto push = [&](int64_t p, bool rev) {
      if (p < 0) return;
      const int32_t* x = part.f.data() + part.off[p]; const int64_t n = part.off[p + 1] - part.off[p];
      for (int64_t i = 0; i < n; ++i) s.f.push_back(rev ? x[n - 1 - i] : x[i]);
    };
    push(a, rev_a); push(b, rev_b);
    anisotropic_weights(s.f.data(), (int64_t)s.f.size(), s.om, s.mk);
    return s;
  };
  for (int64_t i = 0; i < P; ++i) { part.fwd.push_back(seg(i, false, -1, false)); part.bwd.push_back(seg(i, true, -1, false)); }
  for (int64_t i = 0; i + 1 < P; ++i) {
    part.push_fwd.push_back(seg(i, false, i + 1, true));      // :1806-1811
    part.ov_fwd.push_back(seg(i, false, i + 1, true));        // :1835-1836
    part.ov_bwd.push_back(seg(i + 1, false, i, true));        // :1838-1839
  }
  for (int64_t ri = 0; ri + 1 < P; ++ri) { const int64_t i = P - ri - 1; part.push_bwd.push_back(seg(i, false, i - 1, true)); }   // :1813-1820
  part.valid = true;
}

void Plan::partition_pass_segments(int rtype, int inner, std::vector<Segment>& out) {
  ensure_partition();
  const int64_t P = (int64_t)part.fwd.size();
  auto add = [&](const SegList& s) { out.push_back({s.f.data(), (int64_t)s.f.size(), s.om.off.data(), s.om.data.data(), s.mk.off.data(), s.mk.data.data()}); };
  if (rtype == 2) {            // compute_partition_pass, LP_MP.h:1932-1963
    for (int64_t i = 0; i < P; ++i) {
      for (int it = 0; it < inner; ++it) { add(part.fwd[i]); add(part.bwd[i]); }
      if (i < P - 1) add(part.push_fwd[i]);
    }
    for (int64_t ri = 0; ri < P; ++ri) {
      const int64_t i = P - ri - 1;
      for (int it = 0; it < inner; ++it) { add(part.fwd[i]); add(part.bwd[i]); }
      if (i != 0) add(part.push_bwd[ri]);
    }
  } else {                     // compute_overlapping_partition_pass, LP_MP.h:2024-2050
    for (int64_t i = 0; i + 1 < P; ++i) {
      for (int it = 0; it < inner; ++it) { add(part.ov_fwd[i]); add(part.ov_bwd[i]); }
      add(part.ov_fwd[i]);
    }
    for (int64_t ri = 1; ri < P; ++ri) {
      const int64_t i = P - ri - 1;
      for (int it = 0; it < inner; ++it) { add(part.ov_bwd[i]); add(part.ov_fwd[i]); }
      add(part.ov_bwd[i]);
    }
  }
}

void Plan::make_schedule(const int32_t* factors, int64_t n, const int64_t* om_off, const double* om,
                         const int64_t* mk_off, const uint8_t* mk, Schedule& out) const {
  make_schedule(std::vector<Segment>{Segment{factors, n, om_off, om, mk_off, mk}}, false, out);
}

}  // namespace lpmp
