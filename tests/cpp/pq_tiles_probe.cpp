// The skewed tiled order of the peer-minima launches (lp_mp_amd/csrc/order.cpp skewed_tile_order), host only:
//   g++ -std=c++17 -O2 -I lp_mp_amd/csrc tests/cpp/pq_tiles_probe.cpp lp_mp_amd/csrc/order.cpp -lpthread
// The step records, the expansion of a periodic template and the hazard proof of the published minima are those of
// peer_minima_probe.cpp (included, its main renamed).  For 32-label grids of 24 x 24, 40 x 24 and 33 x 47, tiles of 3 to 6 blocks, 1 and
// 3 sub-bands, lags 1 and 2, depths 2, 4, 8 and 16, and 4 to 33 passes, the tables joined_pass_tables emits are checked: every
// (step, block) exactly once, every dependency before its ticket, the periodic template accepted and expanded as the kernel expands
// it, the reader of every slot after its publisher and the next publisher after the reader; one sub-band gives tiled_order's tables
// and no tiles give band_order's.  Prints "pq tiles ok" and exits 0, or names the first failed check and exits 1.
#define main peer_minima_probe_main
#include "peer_minima_probe.cpp"
#undef main

static int64_t tables_checked = 0;

// every (step, block) once, every dependency earlier
static void check_tables(const RotationInfo& ri, const Launch& l, int n, const char* what) {
  const int ns = 2 * n + 1;
  int64_t want = 0;
  std::vector<std::vector<uint8_t>> seen((size_t)ns);
  for (int st = 0; st < ns; ++st) { seen[st].assign((size_t)ri.t[st == 0 ? 0 : st == ns - 1 ? 3 : (st & 1) ? 1 : 2].nb, 0); want += (int64_t)seen[st].size(); }
  CHECK(l.N == want, "%s, %d passes: %lld tickets for %lld blocks", what, n, (long long)l.N, (long long)want);
  for (int64_t t = 0; t < l.N && !failures; ++t) {
    CHECK(l.step[t] >= 0 && l.step[t] < ns && l.block[t] >= 0 && l.block[t] < (int32_t)seen[l.step[t]].size(), "%s, %d passes: ticket %lld out of range", what, n, (long long)t);
    if (failures) return;
    CHECK(!seen[l.step[t]][l.block[t]], "%s, %d passes: step %d block %d twice", what, n, l.step[t], l.block[t]);
    seen[l.step[t]][l.block[t]] = 1;
    for (int32_t d : l.dep[t]) CHECK(d >= 0 && d < t, "%s, %d passes: ticket %lld depends on ticket %d", what, n, (long long)t, d);
  }
  ++tables_checked;
}

static bool same(const TicketOrder& a, const TicketOrder& b) { return a.tk_step == b.tk_step && a.tk_block == b.tk_block && a.new_of == b.new_of && a.group_begin == b.group_begin; }

int main() {
  const std::pair<int, int> grids[] = {{24, 24}, {40, 24}, {33, 47}};
  const int passes[] = {4, 5, 8, 9, 12, 13, 20, 33};
  for (const auto& hw : grids) {
    const std::string name = std::to_string(hw.first) + " x " + std::to_string(hw.second);
    const Steps s = make_steps(grid(hw.first, hw.second));
    const RotationInfo ri = plan_rotation_chain(s.fb, s.bf, s.nf);
    CHECK(ri.valid && ri.peer_minima, "%s: '%s'", name.c_str(), ri.peer_minima_why.c_str());
    CHECK(ri.t[0].nb == ri.t[2].nb && ri.t[3].nb == ri.t[2].nb, "%s: block counts", name.c_str());
    if (failures) break;
    // the geometry figures: a W step moves more than its tables, the consuming steps no table at all
    const PqGeometry pg = peer_minima_geometry(ri);
    CHECK(pg.step_bytes[1] > ri.t[1].bytes && pg.step_bytes[2] < ri.t[2].bytes && pg.step_bytes[0] == ri.t[0].bytes && pg.tile_blocks >= 1 && pg.sub >= 1, "%s: geometry", name.c_str());
    for (int T : {3, 4, 6}) {
      const TileSet ts = make_tiles(ri, T);
      {   // the delayed shares over 16 steps: the first 8 are make_tiles' own, none decreases from a step to the step two later
        TileSet deep = ts;
        extend_tile_delays(ri, deep);
        for (int i = 0; i < 8; ++i) CHECK(deep.delayed[i] == ts.delayed[i], "%s: delayed[%d] changed", name.c_str(), i);
        for (int i = 1; i < TILE_STEPS_MAX; ++i) CHECK(deep.delayed[i] >= 0 && deep.delayed[i] <= 1 && (i < 2 || deep.delayed[i] >= deep.delayed[i - 2]), "%s: delayed[%d]", name.c_str(), i);
      }
      for (int depth : {2, 4, 8, TILE_STEPS_MAX}) for (int sub : {1, 3}) for (int lag : {1, 2}) for (int gap : {0, 2}) {
        if (sub == 1 && (lag == 2 || gap == 2)) continue;          // (one sub-band has no lag and no gap)
        if (gap == 2 && lag == 1 && T != 4) continue;              // (a gap above the lag: on one tile size)
        const JoinedOrder ord{1, 3, depth, &ts, sub, lag, gap};
        char what[160];
        std::snprintf(what, sizeof what, "%s, tiles of %d, depth %d, %d sub-bands, lag %d, gap %d", name.c_str(), T, depth, sub, lag, gap);
        for (int n : passes) {
          // the hazard proof walks the dependency graph per slot: every order on the smallest grid, the others at three pass counts
          const bool slots = hw.first == 24 || n == 5 || n == 13 || n == 33;
          JoinedTables jt;
          std::string why = joined_pass_tables(ri, ord, n, false, jt, nullptr);
          CHECK(why.empty() && jt.sub == sub, "%s, %d passes: '%s', %d sub-bands", what, n, why.c_str(), jt.sub);
          if (!why.empty()) continue;
          const Launch l = expand(jt, depth, 0);
          check_tables(ri, l, n, what);
          if (slots && !failures) check_slots(s, ri, l, n, what);
          {   // one sub-band is the tiled order, ticket for ticket; the order called directly gives the emitted tables
            TicketOrder a, b;
            skewed_tile_order(ri, n, ts, depth, sub, lag, ord.sub_gap, a);
            CHECK(a.tk_step == jt.tk_launch && a.tk_block == jt.tk_block, "%s, %d passes: emitted tables", what, n);
            if (sub == 1) { tiled_order(ri, n, ts, depth, b); CHECK(same(a, b), "%s, %d passes: one sub-band is not the tiled order", what, n); }
          }
          const int tail = (2 * n + 1) % depth, n_tmpl = (3 * depth + tail - 1) / 2;
          if (n < n_tmpl || n <= 7) continue;
          JoinedTables tp;
          why = joined_pass_tables(ri, ord, n_tmpl, true, tp, nullptr);     // (throws where the template is not periodic)
          CHECK(why.empty() && tp.per_len > 0 && tp.ring == 3 * tp.per_len, "%s, template of %d passes: '%s'", what, n_tmpl, why.c_str());
          const int extra = (n - n_tmpl) / (depth / 2);
          CHECK(n_tmpl + extra * (depth / 2) == n, "%s: %d passes do not fit the template of %d", what, n, n_tmpl);
          if (!why.empty() || failures) continue;
          const Launch lp = expand(tp, depth, extra);
          check_tables(ri, lp, n, what);
          if (slots && !failures) check_slots(s, ri, lp, n, what);
        }
      }
    }
    // the wide consume form (blocks of PQ_WIDE_RECORDS records in H, K, T: relations of its own): every block once, dependencies
    // backwards, the template periodic (the slots are checked on the plan's own relations above)
    const RotationInfo rw = plan_rotation_chain(s.fb, s.bf, s.nf, PQ_WIDE_RECORDS);
    CHECK(rw.valid && rw.t[2].nb < ri.t[2].nb && rw.t[0].nb == rw.t[2].nb && rw.t[3].nb == rw.t[2].nb, "%s: wide relations", name.c_str());
    if (rw.valid) {
      const TileSet tw = make_tiles(rw, 4);
      for (int depth : {4, 8, TILE_STEPS_MAX}) for (int gap : {0, 2}) {
        const JoinedOrder ord{1, 3, depth, &tw, 3, 2, gap};
        for (int n : passes) {
          JoinedTables jt;
          std::string why = joined_pass_tables(rw, ord, n, false, jt, nullptr);
          CHECK(why.empty() && jt.sub == 3, "%s, wide, depth %d, %d passes: '%s'", name.c_str(), depth, n, why.c_str());
          if (why.empty()) check_tables(rw, expand(jt, depth, 0), n, "wide consume blocks");
          const int tail = (2 * n + 1) % depth, n_tmpl = (3 * depth + tail - 1) / 2;
          if (n < n_tmpl || n <= 7) continue;
          JoinedTables tp;
          why = joined_pass_tables(rw, ord, n_tmpl, true, tp, nullptr);
          CHECK(why.empty() && tp.per_len > 0, "%s, wide, template of %d passes: '%s'", name.c_str(), n_tmpl, why.c_str());
          if (why.empty()) check_tables(rw, expand(tp, depth, (n - n_tmpl) / (depth / 2)), n, "wide consume blocks, periodic");
        }
      }
    }
    // without tiles the emitted tables are the band order's, whatever the sub-band fields say
    for (int n : {4, 9}) {
      JoinedOrder ord{8, 2, 4, nullptr, 3, 2};
      JoinedTables jt;
      const std::string why = joined_pass_tables(ri, ord, n, false, jt, nullptr);
      std::vector<int64_t> nb;
      for (int st = 0; st < 2 * n + 1; ++st) nb.push_back(ri.t[st == 0 ? 0 : st == 2 * n ? 3 : (st & 1) ? 1 : 2].nb);
      TicketOrder b;
      band_order(nb, 8, jt.lag, 4, b);
      CHECK(why.empty() && jt.sub == 1 && b.tk_step == jt.tk_launch && b.tk_block == jt.tk_block, "%s, %d passes: band order", name.c_str(), n);
    }
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("pq tiles ok (%lld tables, %lld ordered pairs)\n", (long long)tables_checked, (long long)pairs_checked);
  return 0;
}
