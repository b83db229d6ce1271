// schedule_probe.cpp — test code: the planner's real Schedule (plan.cpp, chain_plan.cpp, order.cpp), seen from Python as flat
// arrays.  Built by tests/test_schedule_hazards_host.py with g++ alone; nothing under lp_mp_amd/ includes or links it.  It
// copies, it never judges: footprints, conflicts and reachability are computed in tests/schedule_hazards.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "plan.hpp"

using namespace lpmp;

namespace {

// one row per member of ChainSettings (plan.hpp), in declaration order: the test counts the struct's members against this table
struct Knob { const char* field; const char* env; };
const Knob KNOBS[] = {
    {"chain_min", "LPMP_CHAIN_MIN"},
    {"chain_all", "LPMP_CHAIN_ALL"},
    {"no_level_loop", "LPMP_NO_LEVEL_LOOP"},
    {"no_blocked_passes", "LPMP_NO_BLOCKED_PASSES"},
    {"band_min_bytes", "LPMP_BAND_MIN_BYTES"},
    {"band_min_set", "LPMP_BAND_MIN_BYTES"},
    {"band_bytes", "LPMP_BAND_BYTES"},
    {"heavy_bytes", "LPMP_CHAIN_HEAVY_BYTES"},
    {"no_mailbox", "LPMP_NO_MAILBOX"},
    {"verbose", "LPMP_ROT_VERBOSE"},
};
constexpr int N_KNOBS = (int)(sizeof(KNOBS) / sizeof(KNOBS[0]));

void set_num(const char* name, int64_t v) { setenv(name, std::to_string((long long)v).c_str(), 1); }
void set_flag(const char* name, bool on) { if (on) setenv(name, "1", 1); else unsetenv(name); }

// the environment chain_settings_from_env reads, from explicit settings (values in KNOBS order)
void apply_settings(const int64_t* v) {
  set_num("LPMP_CHAIN_MIN", v[0]);
  set_flag("LPMP_CHAIN_ALL", v[1] != 0);
  set_flag("LPMP_NO_LEVEL_LOOP", v[2] != 0);
  set_flag("LPMP_NO_BLOCKED_PASSES", v[3] != 0);
  if (v[5] != 0) set_num("LPMP_BAND_MIN_BYTES", v[4]); else unsetenv("LPMP_BAND_MIN_BYTES");
  set_num("LPMP_BAND_BYTES", v[6]);
  set_num("LPMP_CHAIN_HEAVY_BYTES", v[7]);
  set_flag("LPMP_NO_MAILBOX", v[8] != 0);
  set_flag("LPMP_ROT_VERBOSE", v[9] != 0);
}
void clear_settings() { for (const Knob& k : KNOBS) unsetenv(k.env); }
bool settings_took(const int64_t* v) {
  const ChainSettings cs = chain_settings_from_env();
  return cs.chain_min == v[0] && cs.chain_all == (v[1] != 0) && cs.no_level_loop == (v[2] != 0) && cs.no_blocked_passes == (v[3] != 0) &&
         (v[5] == 0 || cs.band_min_bytes == v[4]) && cs.band_min_set == (v[5] != 0) && cs.band_bytes == v[6] && cs.heavy_bytes == v[7] &&
         cs.no_mailbox == (v[8] != 0) && cs.verbose == (v[9] != 0);
}

struct Probe {
  Plan plan;
  Schedule s;
  std::string err;
  // the update sequence the schedule was planned from
  std::vector<int64_t> seg_n, om_off{0}, mk_off{0};
  std::vector<int32_t> factor;
  std::vector<double> om;
  std::vector<uint8_t> mk;
  std::vector<int64_t> rec_launch;
};

void keep_sequence(Probe& p, const std::vector<Plan::Segment>& segs) {
  p.seg_n.clear(); p.om_off.assign(1, 0); p.mk_off.assign(1, 0); p.factor.clear(); p.om.clear(); p.mk.clear();
  for (const auto& sg : segs) {
    p.seg_n.push_back(sg.n);
    for (int64_t i = 0; i < sg.n; ++i) {
      p.factor.push_back(sg.factors[i]);
      for (int64_t k = sg.om_off[i]; k < sg.om_off[i + 1]; ++k) p.om.push_back(sg.om[k]);
      for (int64_t k = sg.mk_off[i]; k < sg.mk_off[i + 1]; ++k) p.mk.push_back(sg.mk[k]);
      p.om_off.push_back((int64_t)p.om.size()); p.mk_off.push_back((int64_t)p.mk.size());
    }
  }
}

// the packet copy of op k of record i (nullptr: its launch has no packets)
const Op* packet_op(const Probe& p, int64_t i, int k) {
  const int64_t li = p.rec_launch[(size_t)i];
  if (li < 0) return nullptr;
  const LevelRange& lr = p.s.launches[(size_t)li];
  if (lr.stride <= 0) return nullptr;
  return p.s.packets.data() + lr.pk_begin + (i - lr.begin) * lr.stride + 1 + k;
}

// the packet header of record i (nullptr: its launch has no packets)
const UpdRec* packet_rec(const Probe& p, int64_t i) {
  const Op* first = packet_op(p, i, 0);
  return first ? reinterpret_cast<const UpdRec*>(first - 1) : nullptr;
}
constexpr int64_t NO_PACKET = INT64_MIN;

template <class F>
int64_t emit(int64_t n, int64_t* out, F&& f) { if (out) for (int64_t i = 0; i < n; ++i) out[i] = f(i); return n; }

}  // namespace

extern "C" {

int probe_n_settings() { return N_KNOBS; }
const char* probe_setting_name(int i) { return i >= 0 && i < N_KNOBS ? KNOBS[i].field : nullptr; }

void* probe_create(const lpmp_model* m, int force_generic, int64_t mailbox_budget_bytes, char* err, int err_len) {
  Probe* p = new Probe();
  try {
    p->plan.build(*m);
    p->plan.force_generic = force_generic != 0;
    p->plan.mailbox_budget_bytes = mailbox_budget_bytes;
    return p;
  } catch (const std::exception& e) {
    if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", e.what());
    delete p;
    return nullptr;
  }
}
void probe_destroy(void* h) { delete static_cast<Probe*>(h); }
const char* probe_error(void* h) { return static_cast<Probe*>(h)->err.c_str(); }

// source 0: the given segments (concatenated; om_off / mk_off restart at 0 in every segment and have n + 1 entries each);
// source 2 / 3: Plan::partition_pass_segments(source, inner).  settings: N_KNOBS values in the order of probe_setting_name.
int probe_plan(void* h, int source, int inner, int n_seg, const int64_t* seg_n, const int32_t* factors, const int64_t* om_off, const double* om,
               const int64_t* mk_off, const uint8_t* mk, int fuse, const int64_t* settings, int n_settings) {
  Probe& p = *static_cast<Probe*>(h);
  p.err.clear();
  if (n_settings != N_KNOBS) { p.err = "settings: wrong number of values"; return -1; }
  try {
    std::vector<Plan::Segment> segs;
    if (source == 0) {
      for (int s = 0; s < n_seg; ++s) {
        segs.push_back({factors, seg_n[s], om_off, om, mk_off, mk});
        om += om_off[seg_n[s]]; mk += mk_off[seg_n[s]];
        factors += seg_n[s]; om_off += seg_n[s] + 1; mk_off += seg_n[s] + 1;
      }
    } else {
      p.plan.partition_pass_segments(source, inner, segs);
    }
    keep_sequence(p, segs);
    apply_settings(settings);
    if (!settings_took(settings)) { clear_settings(); p.err = "settings: the environment did not give them back"; return -1; }
    try { p.plan.make_schedule(segs, fuse != 0, p.s); } catch (...) { clear_settings(); throw; }
    clear_settings();
    p.rec_launch.assign(p.s.recs.size(), -1);
    for (size_t li = 0; li < p.s.launches.size(); ++li)
      for (int64_t i = p.s.launches[li].begin; i < p.s.launches[li].end; ++i) p.rec_launch[(size_t)i] = (int64_t)li;
    return 0;
  } catch (const std::exception& e) {
    p.err = e.what();
    return -1;
  }
}

// integer arrays by name (chain: index into Schedule::chains for the per-chain ones); returns the length, fills out unless null;
// -1: no such array
int64_t probe_get(void* h, const char* name, int chain, int64_t* out) {
  const Probe& p = *static_cast<Probe*>(h);
  const Schedule& s = p.s;
  const std::string n = name;
  const int64_t NR = (int64_t)s.recs.size(), NO = (int64_t)s.ops.size(), NL = (int64_t)s.launches.size(), NC = (int64_t)s.chains.size();
  // per record
  if (n == "rec_launch") return emit(NR, out, [&](int64_t i) { return p.rec_launch[(size_t)i]; });
  if (n == "rec_level") return emit(NR, out, [&](int64_t i) { return p.rec_launch[(size_t)i] < 0 ? (int64_t)-1 : (int64_t)s.launches[(size_t)p.rec_launch[(size_t)i]].level; });
  if (n == "rec_class") return emit(NR, out, [&](int64_t i) { return p.rec_launch[(size_t)i] < 0 ? (int64_t)-1 : (int64_t)s.launches[(size_t)p.rec_launch[(size_t)i]].kclass; });
  if (n == "rec_factor") return emit(NR, out, [&](int64_t i) { return (int64_t)s.recs[(size_t)i].factor; });
  if (n == "rec_n_recv") return emit(NR, out, [&](int64_t i) { return (int64_t)s.recs[(size_t)i].n_recv; });
  if (n == "rec_n_send") return emit(NR, out, [&](int64_t i) { return (int64_t)s.recs[(size_t)i].n_send; });
  if (n == "rec_op_begin") return emit(NR, out, [&](int64_t i) { return (int64_t)s.recs[(size_t)i].op_begin; });
  if (n == "rec_kind_flags") return emit(NR, out, [&](int64_t i) { return (int64_t)s.recs[(size_t)i].kind_flags; });
  // where the record's factor lies in the dual / const arrays, in elements (read-only: tests/test_far_offsets_host.py)
  if (n == "rec_dual_off") return emit(NR, out, [&](int64_t i) { return s.recs[(size_t)i].dual_off; });
  if (n == "rec_const_off") return emit(NR, out, [&](int64_t i) { return s.recs[(size_t)i].const_off; });
  // ... and the same words of the record's packet header (NO_PACKET: its launch has no packets)
  if (n == "pk_rec_dual_off") return emit(NR, out, [&](int64_t i) { const UpdRec* h = packet_rec(p, i); return h ? h->dual_off : NO_PACKET; });
  if (n == "pk_rec_const_off") return emit(NR, out, [&](int64_t i) { const UpdRec* h = packet_rec(p, i); return h ? h->const_off : NO_PACKET; });
  if (n == "no_packet") return emit(1, out, [&](int64_t) { return NO_PACKET; });
  // per op (of Schedule::ops)
  if (n == "op_peer") return emit(NO, out, [&](int64_t i) { return (int64_t)s.ops[(size_t)i].peer; });
  if (n == "op_side") return emit(NO, out, [&](int64_t i) { return (int64_t)((s.ops[(size_t)i].info >> 5) & 1); });
  if (n == "op_role") return emit(NO, out, [&](int64_t i) { return (int64_t)((s.ops[(size_t)i].info >> 4) & 1); });
  if (n == "op_code") return emit(NO, out, [&](int64_t i) { return (int64_t)(s.ops[(size_t)i].info & 15); });
  if (n == "op_pad") return emit(NO, out, [&](int64_t i) { return (int64_t)s.ops[(size_t)i].pad; });
  if (n == "op_omega_bits") return emit(NO, out, [&](int64_t i) { int64_t b; std::memcpy(&b, &s.ops[(size_t)i].omega, 8); return b; });
  if (n == "op_peer_dual") return emit(NO, out, [&](int64_t i) { return s.ops[(size_t)i].peer_dual; });
  if (n == "op_peer_const") return emit(NO, out, [&](int64_t i) { return s.ops[(size_t)i].peer_const; });
  // the packet copies of the same two words (a mailbox send's peer_const is its row: op_mailbox_row); NO_PACKET where there is none
  if (n == "pk_op_peer_dual" || n == "pk_op_peer_const") {
    const bool dual = n == "pk_op_peer_dual";
    if (out) {
      for (int64_t i = 0; i < NO; ++i) out[i] = NO_PACKET;
      for (int64_t r = 0; r < NR; ++r) {
        const UpdRec& rec = s.recs[(size_t)r];
        for (int k = 0; k < rec.n_recv + rec.n_send; ++k)
          if (const Op* po = packet_op(p, r, k)) out[rec.op_begin + k] = dual ? po->peer_dual : po->peer_const;
      }
    }
    return NO;
  }
  // the packet copies: OP_MAILBOX and the row (send: peer_const, receive: the bits of omega); -1 where there is no packet or no bit
  if (n == "op_mailbox_row") {
    if (out) {
      for (int64_t i = 0; i < NO; ++i) out[i] = -1;
      for (int64_t r = 0; r < NR; ++r) {
        const UpdRec& rec = s.recs[(size_t)r];
        for (int k = 0; k < rec.n_recv + rec.n_send; ++k) {
          const Op* po = packet_op(p, r, k);
          if (!po || !(po->info & OP_MAILBOX)) continue;
          int64_t row;
          if (k < rec.n_recv) std::memcpy(&row, &po->omega, 8); else row = po->peer_const;
          out[rec.op_begin + k] = row;
        }
      }
    }
    return NO;
  }
  // per launch
  if (n == "launch_class") return emit(NL, out, [&](int64_t i) { return (int64_t)s.launches[(size_t)i].kclass; });
  if (n == "launch_begin") return emit(NL, out, [&](int64_t i) { return s.launches[(size_t)i].begin; });
  if (n == "launch_end") return emit(NL, out, [&](int64_t i) { return s.launches[(size_t)i].end; });
  if (n == "launch_level") return emit(NL, out, [&](int64_t i) { return (int64_t)s.launches[(size_t)i].level; });
  if (n == "launch_stride") return emit(NL, out, [&](int64_t i) { return (int64_t)s.launches[(size_t)i].stride; });
  if (n == "launch_n_recv") return emit(NL, out, [&](int64_t i) { return s.launches[(size_t)i].n_recv; });
  if (n == "launch_bytes") return emit(NL, out, [&](int64_t i) { return s.launches[(size_t)i].bytes; });
  if (n == "launch_n_sh") return emit(NL, out, [&](int64_t i) { return (int64_t)s.launches[(size_t)i].n_sh; });
  if (n == "plain_launches") return emit((int64_t)s.plain_launches.size(), out, [&](int64_t i) { return (int64_t)s.plain_launches[(size_t)i]; });
  if (n == "n_levels") return emit(1, out, [&](int64_t) { return s.n_levels; });
  // per chain
  if (n == "chain_class") return emit(NC, out, [&](int64_t i) { return (int64_t)s.chains[(size_t)i].kclass; });
  if (n == "chain_block_records") return emit(NC, out, [&](int64_t i) { return (int64_t)kc_block_records(s.chains[(size_t)i].kclass); });
  if (n == "chain_level_loop") return emit(NC, out, [&](int64_t i) { return (int64_t)s.chains[(size_t)i].level_loop; });
  if (n == "chain_banded") return emit(NC, out, [&](int64_t i) { return (int64_t)s.chains[(size_t)i].banded; });
  if (n == "chain_valid") return emit(NC, out, [&](int64_t i) { return (int64_t)s.chains[(size_t)i].valid; });
  if (n == "chain_mailbox_rows") return emit(NC, out, [&](int64_t i) { return s.chains[(size_t)i].mailbox_rows; });
  if (n == "chain_mailbox_width") return emit(NC, out, [&](int64_t i) { return (int64_t)s.chains[(size_t)i].mailbox_width; });
  if (n == "mailbox_sends") return emit(1, out, [&](int64_t) { return (int64_t)MAILBOX_SENDS; });
  if (chain >= 0 && chain < NC) {
    const ChainPlan& c = s.chains[(size_t)chain];
    if (n == "cl_rec_begin") return emit((int64_t)c.launches.size(), out, [&](int64_t i) { return c.launches[(size_t)i].rec_begin; });
    if (n == "cl_count") return emit((int64_t)c.launches.size(), out, [&](int64_t i) { return c.launches[(size_t)i].count; });
    if (n == "cl_ticket0") return emit((int64_t)c.launches.size(), out, [&](int64_t i) { return (int64_t)c.launches[(size_t)i].ticket0; });
    if (n == "cl_flags") return emit((int64_t)c.launches.size(), out, [&](int64_t i) { return (int64_t)c.launches[(size_t)i].flags; });
    if (n == "tk_launch") return emit((int64_t)c.tk_launch.size(), out, [&](int64_t i) { return (int64_t)c.tk_launch[(size_t)i]; });
    if (n == "tk_block") return emit((int64_t)c.tk_block.size(), out, [&](int64_t i) { return (int64_t)c.tk_block[(size_t)i]; });
    if (n == "dep_off") return emit((int64_t)c.dep_off.size(), out, [&](int64_t i) { return (int64_t)c.dep_off[(size_t)i]; });
    if (n == "dep") return emit((int64_t)c.dep.size(), out, [&](int64_t i) { return (int64_t)c.dep[(size_t)i]; });
  }
  // the sequence
  if (n == "seg_n") return emit((int64_t)p.seg_n.size(), out, [&](int64_t i) { return p.seg_n[(size_t)i]; });
  if (n == "seq_factor") return emit((int64_t)p.factor.size(), out, [&](int64_t i) { return (int64_t)p.factor[(size_t)i]; });
  if (n == "seq_om_off") return emit((int64_t)p.om_off.size(), out, [&](int64_t i) { return p.om_off[(size_t)i]; });
  if (n == "seq_mk_off") return emit((int64_t)p.mk_off.size(), out, [&](int64_t i) { return p.mk_off[(size_t)i]; });
  if (n == "seq_mk") return emit((int64_t)p.mk.size(), out, [&](int64_t i) { return (int64_t)p.mk[(size_t)i]; });
  if (n == "seq_om_bits") return emit((int64_t)p.om.size(), out, [&](int64_t i) { int64_t b; std::memcpy(&b, &p.om[(size_t)i], 8); return b; });
  return -1;
}

}  // extern "C"
