// chain_plan.cpp — see plan.hpp.  The chain plans of a deep schedule (kernels.hip, chain executor): its launches become
// persistent launches, one per kernel class, with tickets and predecessor lists; message vectors of the packed dense / Potts
// classes travel through a mailbox; many tiny levels of the generic / lane-per-factor classes become the level loop; a few
// HBM-sized steps get the banded Infinity-Cache order.  Host only: plan.cpp hands over the records, launches and packets.
#include "plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <stdexcept>

namespace lpmp {

static_assert(MAILBOX_SENDS == 4, "the forwarding hints of plan.cpp (Op::pad) are planned for four receives: a mailbox form that "
                                  "forwards fewer results in registers needs them retracted in the launches of its chains again");

ChainSettings chain_settings_from_env() {
  ChainSettings cs;
  if (const char* v = std::getenv("LPMP_CHAIN_MIN")) cs.chain_min = (int64_t)std::atoll(v);
  const char* all = std::getenv("LPMP_CHAIN_ALL");
  cs.chain_all = all && std::atoi(all) != 0;
  cs.no_level_loop = std::getenv("LPMP_NO_LEVEL_LOOP") != nullptr;
  cs.no_blocked_passes = std::getenv("LPMP_NO_BLOCKED_PASSES") != nullptr;
  if (const char* v = std::getenv("LPMP_BAND_MIN_BYTES")) { cs.band_min_bytes = std::atoll(v); cs.band_min_set = true; }
  if (const char* v = std::getenv("LPMP_BAND_BYTES")) cs.band_bytes = std::max<int64_t>(1, std::atoll(v));
  if (const char* v = std::getenv("LPMP_CHAIN_HEAVY_BYTES")) cs.heavy_bytes = std::atoll(v);
  cs.no_mailbox = std::getenv("LPMP_NO_MAILBOX") != nullptr;
  cs.verbose = std::getenv("LPMP_ROT_VERBOSE") != nullptr;
  return cs;
}

namespace {

[[noreturn]] void fail(const std::string& s) { throw std::runtime_error(s); }

using Edges = std::vector<std::pair<int32_t, int32_t>>;   // (ticket, predecessor ticket)

// every launch of class c stays a plain launch
void keep_plain(Schedule& out, int c) {
  for (size_t li = 0; li < out.launches.size(); ++li) if (out.launches[li].kclass == c) out.plain_launches.push_back((int32_t)li);
}

// A long schedule of HEAVY launches (C4 at full size: 66 levels of ~0.8 GB each, 150 - 300 us per launch) gains nothing from a
// persistent launch — the gaps between its kernels are a per cent of their run time (measured: 12.15 ms per pass as a chain,
// 11.96 ms of kernel time launch by launch) — while its ticket, dependency and mailbox tables are seconds of planning: it
// stays a replayed graph of plain launches.  (Few big steps are the banded case below; LPMP_CHAIN_HEAVY_BYTES moves the bar.)
bool heavy_launches(const Schedule& out, const ChainSettings& cs) {
  if (cs.chain_all || out.launches.size() <= 8) return false;
  int64_t total = 0;
  for (const auto& lr : out.launches) total += lr.bytes;
  return cs.heavy_bytes > 0 && total / (int64_t)out.launches.size() >= cs.heavy_bytes;
}

// tickets per class: one per block of kc_block_records records of a launch, numbered in launch order
struct Tickets {
  std::vector<ChainPlan> cps = std::vector<ChainPlan>(KC_COUNT);
  std::vector<int32_t> of_update, class_of_update;   // per owner update with a record: its ticket and class (else -1)
};
// false: too many tickets for the 32-bit numbering
bool number_tickets(const Schedule& out, int64_t n_updates, const std::vector<int32_t>& rec_upd, Tickets& t) {
  t.of_update.assign(n_updates, -1); t.class_of_update.assign(n_updates, -1);
  std::vector<int32_t> t0(KC_COUNT, 0);
  bool ok = true;
  for (size_t li = 0; li < out.launches.size(); ++li) {
    const auto& lr = out.launches[li];
    ChainPlan& cp = t.cps[lr.kclass];
    cp.kclass = lr.kclass;
    const int gpb = kc_block_records(lr.kclass);
    const int32_t nb = (int32_t)((lr.end - lr.begin + gpb - 1) / gpb);
    cp.launches.push_back({lr.begin, lr.end - lr.begin, lr.pk_begin, lr.stride, t0[lr.kclass]});
    for (int32_t b = 0; b < nb; ++b) { cp.tk_launch.push_back((int32_t)cp.launches.size() - 1); cp.tk_block.push_back(b); }
    for (int64_t i = lr.begin; i < lr.end; ++i) { t.of_update[rec_upd[i]] = t0[lr.kclass] + (int32_t)((i - lr.begin) / gpb); t.class_of_update[rec_upd[i]] = lr.kclass; }
    t0[lr.kclass] += nb;
    if ((int64_t)t0[lr.kclass] + nb > std::numeric_limits<int32_t>::max() / 2) ok = false;
  }
  return ok;
}

// ---- mailbox (kernels.hip, dense_pk_body): in a deep chain of a dense class the vector a send writes is what the neighbour's
// receive one level later waits for.  Through the completion flag that hand-over costs two trips (flag seen, then the vector
// fetched); a send therefore ALSO writes its vector as tagged granules into a mailbox row, the receive polls that row instead of
// the dual array, and the dependency between the two tickets needs no flag.
struct Mailbox {
  std::vector<char> cls = std::vector<char>(KC_COUNT, 0);   // the classes whose chains hand vectors over this way
  // src_rec / src_k: per receive op, the record and send index that LAST wrote the vector the receive reads (the other side of
  // the pairwise factor) — by vector, not by factor: a record that synchronised on a granule has not seen the producer's ticket
  // complete, so no one may read that producer's vector from the dual array on its word
  std::vector<int32_t> src_rec;
  std::vector<int8_t> src_k;
  std::vector<int32_t> rec_of_upd, rec_launch;              // record of every owner update, launch of every record
};

// the packed dense and Potts classes (exact and run-time dims) whose chains are deep enough, every launch in packet form.
// Returns whether there is any.
bool mailbox_classes(const Schedule& out, const std::vector<int64_t>& n_launches_of, bool model_big, const ChainSettings& cs, Mailbox& mb) {
  bool any = false;
  for (int c = 0; c < KC_COUNT; ++c) {
    if (!kc_is_packed(c)) continue;
    // (fewer launches: plain launches, or — a few HBM-sized steps — the banded order; LPMP_CHAIN_MIN lowers the bar for the
    // randomised tests, which then run the mailbox on every small chain)
    bool el = n_launches_of[c] >= cs.chain_min && !(model_big && n_launches_of[c] <= 8 && !cs.no_blocked_passes);
    for (const auto& lr : out.launches) if (lr.kclass == c && lr.stride <= 0) el = false;
    mb.cls[c] = el; any = any || el;
  }
  return any;
}

void mailbox_sources(const Plan& p, const Schedule& out, int64_t n_updates, const std::vector<int32_t>& rec_upd, Mailbox& mb) {
  mb.src_rec.assign(out.ops.size(), -1); mb.src_k.assign(out.ops.size(), -1);
  mb.rec_of_upd.assign(n_updates, -1); mb.rec_launch.assign(out.recs.size(), -1);
  std::vector<int32_t> lw_rec((size_t)2 * p.nf, -1);      // last writer of (factor, side): record ...
  std::vector<int8_t> lw_k((size_t)2 * p.nf, -1);         // ... and its send index (-1: written by a receive)
  for (size_t li = 0; li < out.launches.size(); ++li) {
    const auto& lr = out.launches[li];
    for (int64_t i = lr.begin; i < lr.end; ++i) { mb.rec_of_upd[rec_upd[i]] = (int32_t)i; mb.rec_launch[i] = (int32_t)li; }
    if (!mb.cls[lr.kclass]) continue;
    for (int64_t i = lr.begin; i < lr.end; ++i) {
      const UpdRec& r = out.recs[i];
      const Op* o = out.ops.data() + r.op_begin;
      for (int j = 0; j < r.n_recv; ++j) {
        const int64_t v = (int64_t)2 * o[j].peer + (1 - ((o[j].info >> 5) & 1));
        const int32_t w = lw_rec[v];
        if (w >= 0 && lw_k[v] >= 0 && lw_k[v] < MAILBOX_SENDS && out.launches[mb.rec_launch[w]].kclass == lr.kclass) { mb.src_rec[r.op_begin + j] = w; mb.src_k[r.op_begin + j] = lw_k[v]; }
      }
      for (int j = 0; j < r.n_recv + r.n_send; ++j) {
        const int64_t v = (int64_t)2 * o[j].peer + ((o[j].info >> 5) & 1);
        lw_rec[v] = (int32_t)i; lw_k[v] = j < r.n_recv ? (int8_t)-1 : (int8_t)std::min(j - r.n_recv, 127);
        // a send after a receive of the same record through the same factor whose result was NOT handed over in a
        // register: that receive stored the factor's tracked bound, and the reader's own store of that bound is not
        // ordered after it by a granule -> flag
        if (j >= r.n_recv && o[j].pad == 0)
          for (int a = 0; a < r.n_recv; ++a) if (o[a].peer == o[j].peer) lw_k[v] = -1;
      }
    }
  }
}

// rows of a class <= its receives with a mailbox source (every row is polled by at least one of them): a class whose mailbox
// would not fit the budget keeps its completion flags — decided HERE, before any dependency is dropped
void mailbox_budget(const Schedule& out, int64_t budget_bytes, Mailbox& mb) {
  std::vector<int64_t> rows_upper(KC_COUNT, 0);
  for (const auto& lr : out.launches) {
    if (!mb.cls[lr.kclass]) continue;
    for (int64_t i = lr.begin; i < lr.end; ++i) {
      const UpdRec& r = out.recs[i];
      for (int j = 0; j < r.n_recv; ++j) if (mb.src_rec[r.op_begin + j] >= 0) ++rows_upper[lr.kclass];
    }
  }
  int64_t left = budget_bytes;
  for (int c = 0; c < KC_COUNT; ++c) {
    if (!mb.cls[c]) continue;
    const int64_t bytes = rows_upper[c] * (int64_t)kc_width(c) * 16;
    if (bytes > left) mb.cls[c] = 0; else left -= bytes;
  }
}

// replay the sequence: who touched each factor last.  Fills the (ticket, predecessor) edges of every class the mailbox does not
// cover; false: a dependency runs between two classes
bool replay(const Plan& p, const UpdateView& seq, const Schedule& out, const Tickets& t, const Mailbox& mb, std::vector<Edges>& edges) {
  std::vector<int32_t> toucher(p.nf, -1);
  bool ok = true;
  for (int64_t u = 0; u < seq.n && ok; ++u) {
    const int32_t o = seq.owner[u];
    const int32_t tk = t.of_update[o];
    if (tk < 0) continue;                             // dropped update (no active message)
    const int32_t f = seq.factor[u];
    auto visit = [&](int32_t g, bool via_message = false) {
      const int32_t w = toucher[g];
      if (w >= 0 && w != o) {
        if (t.class_of_update[w] != t.class_of_update[o]) ok = false;      // a dependency between classes
        else if (t.of_update[w] != tk) {
          // covered by the mailbox: o receives through g exactly the vector w's send wrote (and w's own reads of g
          // precede that send in w's program order, so what o writes into g cannot overtake them)
          bool covered = false;
          if (via_message && mb.cls[t.class_of_update[o]]) {
            const UpdRec& r = out.recs[mb.rec_of_upd[o]];
            for (int j = 0; j < r.n_recv; ++j)
              if (out.ops[r.op_begin + j].peer == g && mb.src_rec[r.op_begin + j] == mb.rec_of_upd[w]) covered = true;
          }
          if (!covered) edges[t.class_of_update[o]].emplace_back(tk, t.of_update[w]);
        }
      }
      toucher[g] = o;
    };
    visit(f);
    int64_t ks = 0, kr = 0;
    for (int64_t j = p.fm_off[f]; j < p.fm_off[f + 1]; ++j) {
      const MsgEntry& e = p.fm[j];
      bool active = false;
      if (e.receives && seq.mk[u][kr++]) active = true;
      if (e.sends && seq.om[u][ks++] != 0.0) active = true;
      if (active) visit(e.adjacent, true);
    }
  }
  return ok;
}

// launches of the lane-per-factor class the op-parallel labeling body can run (kernels.hip, label_ops_body): every record a vector
// factor whose ops are labeling messages with it on the left, message length = label count of the table = the factor's size
void label_ops_flags(const Schedule& out, ChainPlan& lp, bool verbose) {
  int dbg_left = 5;
  for (auto& cl : lp.launches) {
    bool fine = true, paired = true;
    for (int64_t i = cl.rec_begin; i < cl.rec_begin + cl.count && fine; ++i) {
      const UpdRec& r = out.recs[i];
      const Op* o = out.ops.data() + r.op_begin;
      const int n = r.n_recv + r.n_send;
      fine = r.n_recv <= 8 && r.n_send <= 8 && (r.kind_flags & 15) == LPMP_F_VECTOR && r.d0 <= SMALL_MAXD;
      for (int a = 0; a < n && fine; ++a) {
        if ((o[a].info & 15) != OP_LABELING || ((o[a].info >> 4) & 1) != 0 || o[a].pd0 > SMALL_MAXD || o[a].len != r.d0 || o[a].pd1 != r.d0) fine = false;
        // the receives run side by side, and so do the sends: no two of a kind on one peer
        for (int b = a + 1; b < n && fine; ++b) if (o[a].peer_dual == o[b].peer_dual && (a < r.n_recv) == (b < r.n_recv)) fine = false;
        // a send into the peer of a receive needs that receive's result: the staged body takes it from LDS where plan.cpp marked
        // the pair (packet_flags: Op::pad, same match table) and otherwise requests the peer's costs together with the receive's,
        // before the receive has rewritten them — one peer through two tables (an iterator-range pass that receives through one
        // and sends through the other) stays on the op-by-op body
        for (int b = r.n_recv; b < n && fine && a < r.n_recv; ++b) if (o[a].peer_dual == o[b].peer_dual && o[b].pad != a + 1) fine = false;
      }
      if (r.n_recv != r.n_send) paired = false;
      for (int a = 0; a < r.n_recv && paired && fine; ++a)
        if (o[a].peer_dual != o[r.n_recv + a].peer_dual || o[a].peer_const != o[r.n_recv + a].peer_const || o[a].pd0 != o[r.n_recv + a].pd0) paired = false;
    }
    if (fine) cl.flags |= CHAIN_LAUNCH_LABEL_OPS | (paired ? CHAIN_LAUNCH_LABEL_PAIRED : 0);
    else if (verbose && dbg_left-- > 0) {
      const UpdRec& r = out.recs[cl.rec_begin]; const Op* o = out.ops.data() + r.op_begin;
      std::fprintf(stderr, "lpmp:   not eligible: first record kind %d d0 %d ops %d+%d; op0 code %d role %d pd0 %d pd1 %d len %d\n", r.kind_flags & 15, r.d0, r.n_recv, r.n_send,
                   (r.n_recv + r.n_send) ? (o[0].info & 15) : -1, (r.n_recv + r.n_send) ? ((o[0].info >> 4) & 1) : -1, (r.n_recv + r.n_send) ? o[0].pd0 : -1, (r.n_recv + r.n_send) ? o[0].pd1 : -1, (r.n_recv + r.n_send) ? o[0].len : -1);
    }
  }
}

// Many TINY levels of the lane-per-factor / generic class (C5 with local triples: 11 887 levels of a dozen one-lane updates):
// one workgroup walks the levels with a workgroup barrier in between — no launch per level, no flags through memory, and the
// duals it hands from level to level stay in its L2.  Wide levels stay plain.
bool level_loop_fits(const Schedule& out, int c, int64_t n_launches, const ChainSettings& cs) {
  int64_t recs_c = 0;
  for (const auto& lr : out.launches) if (lr.kclass == c) recs_c += lr.end - lr.begin;
  return n_launches >= cs.chain_min && recs_c <= (int64_t)kc_block_records(c) * n_launches && !cs.no_level_loop;
}
void level_loop(const Schedule& out, int c, ChainPlan& lp, const ChainSettings& cs) {
  lp.level_loop = true; lp.valid = true;
  if (c == KC_SMALL) label_ops_flags(out, lp, cs.verbose);
  if (cs.verbose) {
    int64_t nf_ = 0, np_ = 0; for (const auto& cl : lp.launches) { nf_ += (cl.flags & CHAIN_LAUNCH_LABEL_OPS) != 0; np_ += (cl.flags & CHAIN_LAUNCH_LABEL_PAIRED) != 0; }
    std::fprintf(stderr, "lpmp: level loop over %zu launches of class %d, %lld of them with one lane per op (%lld paired)\n", lp.launches.size(), c, (long long)nf_, (long long)np_);
  }
  lp.tk_launch.clear(); lp.tk_block.clear(); lp.dep_off.assign(1, 0); lp.dep.clear();
}

// about band_bytes of algorithmic bytes per band; the smallest lag from 3 on that keeps every dependency backwards (the skewed
// band order of order.cpp, one group over all of the class's launches).  Renumbers the tickets and edges; false: no lag does
bool banded_order(int c, int64_t max_bytes, int64_t band_bytes, ChainPlan& cp, Edges& ed) {
  const int gpb = kc_block_records(c);
  std::vector<int64_t> nb;
  int64_t max_nb = 1;                               // (a band narrower than a few blocks cannot keep the dependencies)
  for (const auto& l : cp.launches) { nb.push_back((l.count + gpb - 1) / gpb); max_nb = std::max(max_nb, nb.back()); }
  const int nbands = (int)std::max<int64_t>(2, std::min<int64_t>(max_bytes / band_bytes, max_nb / 4));
  TicketOrder o;
  for (int lg = 3; lg <= 16 && !cp.banded; ++lg) {
    band_order(nb, nbands, lg, (int)nb.size(), o);
    bool fine = true;
    for (const auto& e : ed) if (o.new_of[e.second] >= o.new_of[e.first]) { fine = false; break; }
    if (!fine) continue;
    for (auto& e : ed) { e.first = o.new_of[e.first]; e.second = o.new_of[e.second]; }
    cp.tk_launch.swap(o.tk_step); cp.tk_block.swap(o.tk_block);
    cp.banded = true;
  }
  return cp.banded;
}

// the predecessor lists (CSR over tickets) of the class's edges
void dependency_lists(int64_t n_tickets, Edges& ed, ChainPlan& cp) {
  std::sort(ed.begin(), ed.end());
  ed.erase(std::unique(ed.begin(), ed.end()), ed.end());
  cp.dep_off.assign((size_t)n_tickets + 1, 0);
  for (const auto& e : ed) { if (e.second >= e.first) fail("chain plan: dependency on a later ticket"); cp.dep_off[e.first + 1]++; }
  std::partial_sum(cp.dep_off.begin(), cp.dep_off.end(), cp.dep_off.begin());
  cp.dep.resize(ed.size());
  for (size_t i = 0; i < ed.size(); ++i) cp.dep[i] = ed[i].second;   // sorted by ticket: already in CSR order
}

// rows for the sends some receive polls; the packet copies of both ops carry the row (plan.hpp, OP_MAILBOX)
void mailbox_rows(Schedule& out, const Mailbox& mb, int c, ChainPlan& cp) {
  std::vector<int64_t> row_of_op;                     // per op of out.ops (sends): mailbox row, assigned on first use
  row_of_op.assign(out.ops.size(), -1);
  auto slot_of = [&](int64_t i) { const auto& lr = out.launches[mb.rec_launch[i]]; return out.packets.data() + lr.pk_begin + (i - lr.begin) * lr.stride; };
  int64_t rows = 0;
  for (const auto& cl : cp.launches)
    for (int64_t i = cl.rec_begin; i < cl.rec_begin + cl.count; ++i) {
      const UpdRec& r = out.recs[i];
      for (int j = 0; j < r.n_recv; ++j) {
        const int32_t w = mb.src_rec[r.op_begin + j];
        if (w < 0) continue;
        const UpdRec& rw = out.recs[w];
        const int64_t sop = (int64_t)rw.op_begin + rw.n_recv + mb.src_k[r.op_begin + j];
        if (row_of_op[sop] < 0) {
          row_of_op[sop] = rows++;
          Op& ps = slot_of(w)[1 + rw.n_recv + mb.src_k[r.op_begin + j]];
          ps.peer_const = row_of_op[sop]; ps.info |= OP_MAILBOX;
        }
        Op& pr = slot_of(i)[1 + j];
        std::memcpy(&pr.omega, &row_of_op[sop], sizeof(double)); pr.info |= OP_MAILBOX;
        ++cp.mailbox_receives;
      }
    }
  if (rows > 0) {
    cp.mailbox_rows = rows; cp.mailbox_width = kc_width(c);
    for (auto& cl : cp.launches) cl.flags |= CHAIN_LAUNCH_MAILBOX;
  }
}

}  // namespace

// Dependencies: update u must see the results of the last earlier update that touched u's factor or a factor u touches — the
// same relation the levels were computed from.  Classes are separate launches and cannot wait for each other, so a schedule
// qualifies only if no dependency runs between records of different classes (C5: the Potts grid and the labeling-list factors
// are separate components); classes with few launches stay plain launches.
void plan_chains(const Plan& p, const UpdateView& seq, const std::vector<int32_t>& rec_upd, const ChainSettings& cs, Schedule& out) {
  // a model that fits the 256 MiB Infinity Cache as a whole is re-read on-die by plain launches already
  const bool model_big = cs.band_min_set || (p.f_coff[p.nf] + p.f_doff[p.nf]) * (int64_t)sizeof(double) > ((int64_t)1 << 30);
  bool any_big = false;
  for (const auto& lr : out.launches) any_big = any_big || (model_big && kc_is_dense(lr.kclass) && !kc_is_var(lr.kclass) && lr.n_recv > 0 && lr.bytes >= cs.band_min_bytes);
  if (heavy_launches(out, cs)) return;
  if (out.launches.empty() || !((int64_t)out.launches.size() >= cs.chain_min || (any_big && out.launches.size() >= 2 && !cs.no_blocked_passes))) return;
  std::vector<int64_t> n_launches_of(KC_COUNT, 0);
  bool ok = true;
  for (const auto& lr : out.launches) {
    n_launches_of[lr.kclass]++;
    ok = ok && kc_chain_capable(lr.kclass);
  }
  if (!ok) return;
  Tickets t;
  if (!number_tickets(out, seq.n, rec_upd, t)) return;
  Mailbox mb;
  if (!cs.no_mailbox && mailbox_classes(out, n_launches_of, model_big, cs, mb)) {
    mailbox_sources(p, out, seq.n, rec_upd, mb);
    if (p.mailbox_budget_bytes >= 0) mailbox_budget(out, p.mailbox_budget_bytes, mb);
  }
  std::vector<Edges> edges(KC_COUNT);
  if (!replay(p, seq, out, t, mb, edges)) return;
  for (int c = 0; c < KC_COUNT; ++c) {
    if (n_launches_of[c] == 0) continue;
    ChainPlan& cp = t.cps[c];
    // lane-per-factor and generic records: every dual access of a chain kernel is a device-scope access that goes past the L2,
    // and these bodies issue them one dependent access at a time — measured slower than replaying a hipGraph of plain launches
    // (C5: 202 ms against 188 ms per pass).  The kernels stay available: LPMP_CHAIN_ALL=1.  Those classes get the
    // level loop instead when their levels are tiny.
    if (kc_width(c) == 0 && !cs.chain_all) {
      if (level_loop_fits(out, c, n_launches_of[c], cs)) {
        level_loop(out, c, cp, cs);
        out.chains.push_back(std::move(cp));
      } else {
        keep_plain(out, c);
      }
      continue;
    }
    // A few HBM-sized launches of a dense class (the colour steps of a big grid: forward or backward sweep alone, a fused pass in
    // a weight mode that does not rotate, the per-pass schedule of a multi-GPU part) are worth a chain as well: not for the
    // launch gaps but for the ORDER — consecutive steps read the same pairwise tables, and band j of step l issued at time
    // j + lag * l finds them in the 256 MiB Infinity Cache.
    // (only receives read tables: a directional sweep of a 2-colour grid has ONE such step and gains nothing)
    int64_t max_bytes = 0; int n_table_steps = 0;
    for (const auto& lr : out.launches) if (lr.kclass == c) { max_bytes = std::max(max_bytes, lr.bytes); if (lr.n_recv > 0 && lr.bytes >= cs.band_min_bytes) ++n_table_steps; }
    const bool dense_cls = kc_is_dense(c) && !kc_is_var(c);   // (run-time-dims classes: slower as a banded chain, engine.cpp rotation_chain)
    const bool big_steps = model_big && dense_cls && n_table_steps >= 2 && n_launches_of[c] <= 8 && !cs.no_blocked_passes;
    if (n_launches_of[c] < cs.chain_min && !big_steps) {               // few launches: plain
      keep_plain(out, c);
      continue;
    }
    const int64_t n_tickets = (int64_t)cp.tk_launch.size();
    if (big_steps && n_tickets > 0 && !banded_order(c, max_bytes, cs.band_bytes, cp, edges[c]) && n_launches_of[c] < cs.chain_min) {
      keep_plain(out, c);                                                // no valid order and nothing else to gain: plain launches
      continue;
    }
    dependency_lists(n_tickets, edges[c], cp);
    cp.valid = true;
    if (mb.cls[c]) {
      if (cp.banded) fail("chain plan: mailbox in a banded order");
      mailbox_rows(out, mb, c, cp);
    }
    out.chains.push_back(std::move(cp));
  }
}

}  // namespace lpmp
