// The ticket descriptors of the peer-minima launches (lp_mp_amd/csrc/order.cpp ticket_descriptors), host only:
//   g++ -std=c++17 -O2 -I lp_mp_amd/csrc tests/cpp/pq_desc_probe.cpp lp_mp_amd/csrc/order.cpp -lpthread
// The step records are those of peer_minima_probe.cpp (included, its main renamed).  Templates come from joined_pass_tables on
// 24 x 24 and 33 x 47 grids of 32 labels — band order, tiled order, skewed tiled order, explicit lists and the periodic template,
// each on the plan's own relations and with wide consume blocks — and from hand-made ticket lists with 0, D and D + 1
// dependencies.  For every template ticket and the inline caps 0, 1 and D the descriptor is checked field for field against
// tk_launch, tk_block, dep_off and dep: launch, block, dependency count, the inline entries a prefix of the list, -1 behind them,
// the overflow position where the list continues.  Prints the histogram of dependency counts per ticket of every order and
// "pq desc ok", and exits 0; or names the first failed check and exits 1.
#define main peer_minima_probe_main
#include "peer_minima_probe.cpp"
#undef main

static int64_t tickets_checked = 0, exact_d = 0, over_d = 0, none = 0;

static void check_desc(const std::vector<int32_t>& tk_launch, const std::vector<int32_t>& tk_block, const std::vector<int32_t>& dep_off, const std::vector<int32_t>& dep,
                       int cap, const char* what) {
  const std::vector<int32_t> d = ticket_descriptors(tk_launch, tk_block, dep_off, dep, cap);
  const int D = std::min(std::max(cap, 0), TICKET_DESC_INLINE);
  const size_t N = tk_launch.size();
  CHECK(d.size() == N * TICKET_DESC_WORDS, "%s, cap %d: %zu words for %zu tickets", what, cap, d.size(), N);
  if (failures) return;
  for (size_t t = 0; t < N && !failures; ++t) {
    const int32_t* w = d.data() + t * TICKET_DESC_WORDS;
    const int32_t n = dep_off[t + 1] - dep_off[t], ni = std::min<int32_t>(n, D);
    CHECK(w[TD_LAUNCH] == tk_launch[t] && w[TD_BLOCK] == tk_block[t], "%s, cap %d: ticket %zu launch / block", what, cap, t);
    CHECK(w[TD_NDEPS] == n, "%s, cap %d: ticket %zu has %d dependencies, the descriptor says %d", what, cap, t, n, w[TD_NDEPS]);
    for (int32_t i = 0; i < TICKET_DESC_INLINE; ++i) {
      if (i < ni) CHECK(w[TD_DEPS + i] == dep[(size_t)dep_off[t] + i], "%s, cap %d: ticket %zu inline entry %d", what, cap, t, i);
      else CHECK(w[TD_DEPS + i] == -1, "%s, cap %d: ticket %zu entry %d behind the inline ones", what, cap, t, i);
    }
    // the rest continues the list: inline entries + dep[rest ...] are the ticket's dependencies in order, and end where they end
    CHECK(w[TD_REST] == dep_off[t] + ni && w[TD_REST] + (n - ni) == dep_off[t + 1], "%s, cap %d: ticket %zu overflow position", what, cap, t);
    if (D == TICKET_DESC_INLINE) { exact_d += n == D; over_d += n == D + 1; none += n == 0; }
    ++tickets_checked;
  }
}

static void check_tables(const JoinedTables& jt, const char* what) {
  for (int cap : {0, 1, TICKET_DESC_INLINE, TICKET_DESC_INLINE + 5, -3}) check_desc(jt.tk_launch, jt.tk_block, jt.dep_off, jt.dep, cap, what);
  const std::vector<int64_t> h = ticket_dep_histogram(jt.dep_off, TICKET_DESC_INLINE + 1);
  int64_t total = 0;
  std::printf("%s: dependencies per ticket (0 ... %d, more):", what, TICKET_DESC_INLINE);
  for (int64_t c : h) { std::printf(" %lld", (long long)c); total += c; }
  std::printf("\n");
  CHECK(total == (int64_t)jt.tk_launch.size(), "%s: histogram counts %lld of %zu tickets", what, (long long)total, jt.tk_launch.size());
}

int main() {
  // hand-made lists: tickets with 0, 1, D - 1, D, D + 1 and 3 D dependencies, each on all earlier tickets it can name
  {
    const int D = TICKET_DESC_INLINE;
    std::vector<int32_t> tl, tb, off{0}, dep;
    const int counts[] = {0, 0, 1, D - 1, D, D + 1, 0, 3 * D, D, D + 1, 1, D + 1};
    int32_t t = 0;
    for (int rep = 0; rep < 4; ++rep)
      for (int c : counts) {
        tl.push_back(t % 5); tb.push_back(7 * t + 1);
        for (int i = 0; i < c; ++i) dep.push_back((int32_t)((t * 31 + i * 17) % std::max<int32_t>(t, 1)));
        off.push_back((int32_t)dep.size());
        ++t;
      }
    for (int cap : {0, 1, 2, D - 1, D}) check_desc(tl, tb, off, dep, cap, "hand-made lists");
    CHECK(exact_d >= 8 && over_d >= 12 && none >= 12, "hand-made lists: %lld tickets with exactly D, %lld with D + 1, %lld with none", (long long)exact_d, (long long)over_d, (long long)none);
    bool threw = false;
    try { off.back() += 1; ticket_descriptors(tl, tb, off, dep, D); } catch (const std::exception&) { threw = true; }
    CHECK(threw, "inconsistent tables are refused");
  }
  const std::pair<int, int> grids[] = {{24, 24}, {33, 47}};
  for (const auto& hw : grids) {
    const Steps s = make_steps(grid(hw.first, hw.second));
    for (int gpb : {0, PQ_WIDE_RECORDS}) {
      const RotationInfo ri = plan_rotation_chain(s.fb, s.bf, s.nf, gpb);
      CHECK(ri.valid && ri.peer_minima, "%d x %d: '%s'", hw.first, hw.second, ri.peer_minima_why.c_str());
      if (failures) break;
      const TileSet ts = make_tiles(ri, 4);
      struct Order { const char* name; JoinedOrder ord; };
      const Order orders[] = {{"band order", {8, 2, 4, nullptr, 1, 1, 0}}, {"tiled order", {1, 3, 8, &ts, 1, 1, 0}}, {"skewed tiled order", {1, 3, 8, &ts, 3, 2, 2}}};
      for (const Order& o : orders) {
        for (int n : {5, 20}) {
          char what[160];
          JoinedTables jt;
          std::string why = joined_pass_tables(ri, o.ord, n, false, jt, nullptr);
          std::snprintf(what, sizeof what, "%d x %d, %s, %s consume blocks, %d passes", hw.first, hw.second, o.name, gpb ? "wide" : "plain", n);
          CHECK(why.empty(), "%s: '%s'", what, why.c_str());
          if (why.empty()) check_tables(jt, what);
          const int depth = o.ord.depth, tail = (2 * n + 1) % depth, n_tmpl = (3 * depth + tail - 1) / 2;
          if (n < n_tmpl || n <= 7) continue;
          JoinedTables tp;
          why = joined_pass_tables(ri, o.ord, n_tmpl, true, tp, nullptr);
          std::snprintf(what, sizeof what, "%d x %d, %s, %s consume blocks, periodic template of %d passes", hw.first, hw.second, o.name, gpb ? "wide" : "plain", n_tmpl);
          CHECK(why.empty() && tp.per_len > 0, "%s: '%s'", what, why.c_str());
          if (why.empty()) check_tables(tp, what);
        }
      }
    }
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("pq desc ok (%lld tickets)\n", (long long)tickets_checked);
  return 0;
}
