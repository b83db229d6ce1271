// engine.cpp — the C ABI of include/lpmp_engine.h: device memory, schedules, launches.
// Host code only; the kernels are in kernels.hip, the prepared sets (read-outs, window, path and forest sets) in prepared.cpp, and
// what the two host files share in engine_state.hpp.  There is NO CPU execution path: every compute
// entry point needs a HIP device and fails with LPMP_ERR_DEVICE otherwise.
#include <hip/hip_runtime.h>

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine_state.hpp"

static thread_local std::string g_error;
const char* lpmp_last_error(void) { return g_error.c_str(); }
int lpmp_set_last_error(const char* msg) { g_error = msg ? msg : ""; return 0; }   // for the other translation units of the library (engine_internal.h)
const char* lpmp_version(void) { return "lp_mp_amd 0.1 (gfx950)"; }
int lpmp_experiment_build(void) { return 0; }   // kept for the ABI: the library has no experimental build

static long long chain_timeout_ticks() {    // LPMP_CHAIN_TIMEOUT_S (default 20 s)
  static const long long v = [] { const char* e = std::getenv("LPMP_CHAIN_TIMEOUT_S"); const double s = e ? std::atof(e) : 20.0; return (long long)(std::max(0.001, s) * 1e8); }();
  return v;
}

static void plan_pass_schedule(lpmp_plan* pl, int mode, bool chains = true) {
  if (pl->have_pass[mode]) return;
  pl->p.ensure_weights(mode);
  std::vector<Plan::Segment> segs;
  for (int d = 0; d < 2; ++d) {
    const auto& om = pl->p.omega[d][mode];
    const auto& mk = pl->p.mask[d][mode];
    segs.push_back({pl->p.upd[d].data(), (int64_t)pl->p.upd[d].size(), om.off.data(), om.data.data(), mk.off.data(), mk.data.data()});
  }
  pl->p.make_schedule(segs, true, pl->pass_cache[mode], chains);
  pl->have_pass[mode] = true;
}

static void plan_schedule(lpmp_plan* pl, int d, int mode) {
  if (pl->have_sched[d][mode]) return;
  pl->p.ensure_weights(mode);
  const auto& om = pl->p.omega[d][mode];
  const auto& mk = pl->p.mask[d][mode];
  pl->p.make_schedule(pl->p.upd[d].data(), (int64_t)pl->p.upd[d].size(), om.off.data(), om.data.data(), mk.off.data(),
                      mk.data.data(), pl->sched_cache[d][mode]);
  pl->have_sched[d][mode] = true;
}

// Seam between two consecutive passes.  If forward+backward fuses into exactly three steps
//   [H: head of the forward sweep] [W] [T: tail of the backward sweep]
// and backward+forward fuses into [H'] [K] [T'] where K's records are exactly T's receives followed by H's sends
// (same peers, sides, weights, order — checked op by op) and W's are T's' receives followed by H's' sends, then n
// passes are
//   H, W, (K, W) x (n-1), T
// — every record is the same sequence of receives and sends the unfused sweeps execute (plan.cpp, fusion).
// 2-colour orders of bipartite graphs (checkerboard grids) have this shape.
// records of one level keyed by factor
static std::vector<std::pair<int32_t, const UpdRec*>> level_records(const Schedule& s, int level) {
  std::vector<std::pair<int32_t, const UpdRec*>> f;
  for (const auto& lr : s.launches) if (lr.level == level) for (int64_t i = lr.begin; i < lr.end; ++i) f.emplace_back(s.recs[i].factor, &s.recs[i]);
  std::sort(f.begin(), f.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  return f;
}
static bool same_op(const Op& a, const Op& b) {   // everything but the forwarding hint (pad), which is per schedule
  return a.peer_dual == b.peer_dual && a.peer_const == b.peer_const && a.omega == b.omega && a.info == b.info &&
         a.pd0 == b.pd0 && a.pd1 == b.pd1 && a.peer == b.peer && a.len == b.len;
}
// does every record of `joined` (level lj of schedule sj) hold exactly the receives of the same factor's record in
// (sr, lr) followed by the sends of its record in (ss, ls) — same peers, sides, weights, order?
static bool level_is_join(const Schedule& sj, int lj, const Schedule& sr, int lr, const Schedule& ss, int ls) {
  const auto j = level_records(sj, lj), r = level_records(sr, lr), t = level_records(ss, ls);
  if (j.size() != r.size() || j.size() != t.size()) return false;
  for (size_t i = 0; i < j.size(); ++i) {
    if (j[i].first != r[i].first || j[i].first != t[i].first) return false;
    if (i > 0 && j[i].first == j[i - 1].first) return false;   // one record per factor and level
    const UpdRec& a = *j[i].second; const UpdRec& b = *r[i].second; const UpdRec& c = *t[i].second;
    if (b.n_send != 0 || c.n_recv != 0 || a.n_recv != b.n_recv || a.n_send != c.n_send) return false;
    for (int k = 0; k < a.n_recv; ++k) if (!same_op(sj.ops[a.op_begin + k], sr.ops[b.op_begin + k])) return false;
    for (int k = 0; k < a.n_send; ++k) if (!same_op(sj.ops[a.op_begin + a.n_recv + k], ss.ops[c.op_begin + k])) return false;
  }
  return true;
}
static void plan_rotation(lpmp_plan* pl, int mode) {
  if (pl->have_bf[mode]) return;
  pl->have_bf[mode] = true;
  pl->rotation_ok[mode] = false;
  const Schedule& fb = pl->pass_cache[mode];
  if (fb.n_levels != 3 || fb.recs.empty()) return;
  std::vector<Plan::Segment> segs;
  for (int d = 1; d >= 0; --d) {
    const auto& om = pl->p.omega[d][mode];
    const auto& mk = pl->p.mask[d][mode];
    segs.push_back({pl->p.upd[d].data(), (int64_t)pl->p.upd[d].size(), om.off.data(), om.data.data(), mk.off.data(), mk.data.data()});
  }
  Schedule& bf = pl->bf_cache[mode];
  pl->p.make_schedule(segs, true, bf, false);
  // K (middle step of backward+forward) must be exactly "receives of T, then sends of H" factor by factor, and W
  // (middle step of forward+backward) exactly "receives of T', then sends of H'": then H, W, (K, W)^(n-1), T executes
  // the same receives and sends as n unfused passes, in an order that differs only between independent updates
  const bool ok = bf.n_levels == 3 && level_is_join(bf, 2, fb, 3, fb, 1) && level_is_join(fb, 2, bf, 3, bf, 1);
  pl->rotation_ok[mode] = ok;
  if (!ok) bf = Schedule();
}

namespace {

// Copies between caller memory (pageable) and the device go through a pinned staging buffer that this code owns:
// plain memcpy on the calling thread on the host side, hipMemcpyAsync between the pinned buffer and the device on the
// engine's stream, waited for.  Nothing in the HIP runtime then reads or writes caller memory — an asynchronous copy
// straight to / from pageable memory is staged by the runtime on its own, and a handful of runs in ~300 000 randomised
// test runs showed host heap corruption next to freshly freed download buffers.  The engine's stream is
// non-blocking, so the null stream (plain hipMemcpy) would not be ordered with its kernels either.
// Guard regions.  Every host buffer the device or the HIP runtime writes into on the engine's behalf (the staging
// buffer of h2d / d2h, the block of device-written words) sits between two GUARD_BYTES regions holding a fixed
// pattern; the pattern is verified after every staged copy, in lpmp_synchronize and in lpmp_destroy.  A DMA or a
// runtime-side write that runs past its buffer is reported instead of silently landing in a neighbour allocation
// (the host-heap corruption hunt).
constexpr size_t GUARD_BYTES = 4096;
constexpr uint64_t GUARD_WORD = 0xA5C3E1F00F1E3C5AULL;
void guard_fill(void* p) { uint64_t* w = (uint64_t*)p; for (size_t i = 0; i < GUARD_BYTES / 8; ++i) w[i] = GUARD_WORD ^ (uint64_t)i; }
bool guard_ok(const void* p) {
  const uint64_t* w = (const uint64_t*)p;
  for (size_t i = 0; i < GUARD_BYTES / 8; ++i) if (w[i] != (GUARD_WORD ^ (uint64_t)i)) return false;
  return true;
}
// pinned allocation of `bytes` usable bytes with a guard region on either side; returns the usable pointer
char* guarded_host_alloc(size_t bytes) {
  char* raw = nullptr;
  HIP_CHECK(hipHostMalloc((void**)&raw, bytes + 2 * GUARD_BYTES, hipHostMallocDefault));
  guard_fill(raw); guard_fill(raw + GUARD_BYTES + bytes);
  return raw + GUARD_BYTES;
}
void guarded_host_free(char* p) { if (p) (void)hipHostFree(p - GUARD_BYTES); }
bool guarded_ok(const char* p, size_t bytes) { return !p || (guard_ok(p - GUARD_BYTES) && guard_ok(p + bytes)); }

struct Staging {
  char* p = nullptr; size_t bytes = 0;
  void* get(size_t want) {
    if (want > bytes) {
      if (p) { check(); guarded_host_free(p); p = nullptr; bytes = 0; }
      p = guarded_host_alloc(want);
      bytes = want;
    }
    return p;
  }
  void check() const { if (!guarded_ok(p, bytes)) throw DeviceError("guard region of the pinned staging buffer was overwritten"); }
  // (freed only when it grows: it lives as long as the thread, and at thread exit the HIP runtime may already be gone)
};
// small device-written host words (partial sums, counters, flags): one pinned block per engine, taken from a pool
// and given back at destroy — no pinned allocation / free per uploaded model or per engine.  The pools are per thread
// and bounded: beyond POOL_MAX idle entries a returned block is freed / a returned stream destroyed.
constexpr size_t PINNED_WORDS_BYTES = 8 * 1024 + 256;   // 1024 partial sums, then words at +0 (stale counter), +64 (primal flag), +128 ... (chain abort report)
constexpr size_t POOL_MAX = 8;
struct PinnedPool {
  std::vector<char*> free_blocks;
  char* take() {
    if (!free_blocks.empty()) { char* p = free_blocks.back(); free_blocks.pop_back(); return p; }
    return guarded_host_alloc(PINNED_WORDS_BYTES);
  }
  void give(char* p) {
    if (!p) return;
    if (free_blocks.size() < POOL_MAX) free_blocks.push_back(p); else guarded_host_free(p);
  }
};
PinnedPool& pinned_pool() { static thread_local PinnedPool p; return p; }
// streams are pooled per thread and device: a long-lived process that creates and destroys thousands of engines does
// not churn HIP streams (each is a hardware queue with its own signals)
struct StreamPool {
  std::vector<std::pair<int, hipStream_t>> free_streams;
  hipStream_t take(int device) {
    for (size_t i = 0; i < free_streams.size(); ++i)
      if (free_streams[i].first == device) { hipStream_t s = free_streams[i].second; free_streams.erase(free_streams.begin() + i); return s; }
    hipStream_t s = nullptr;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return s;
  }
  void give(int device, hipStream_t s) {
    if (!s) return;
    // LPMP_STREAM_POOL=0: destroy instead of pooling — the round-1 behaviour, kept as the A/B switch of the host-heap
    // corruption hunt (tests/fuzz_split.py)
    static const bool pooling = [] { const char* v = std::getenv("LPMP_STREAM_POOL"); return !(v && v[0] == '0'); }();
    if (pooling && free_streams.size() < POOL_MAX) free_streams.emplace_back(device, s); else (void)hipStreamDestroy(s);
  }
};
StreamPool& stream_pool() { static thread_local StreamPool p; return p; }
Staging& staging() { static thread_local Staging s; return s; }

// LPMP_DIRECT_COPIES=1: asynchronous copies straight to / from the caller's (pageable) memory followed by a stream
// synchronise — the round-1 original, kept as an A/B switch of the host-heap corruption hunt
bool direct_copies() { static const bool v = [] { const char* e = std::getenv("LPMP_DIRECT_COPIES"); return e && e[0] == '1'; }(); return v; }
}  // namespace

// (declared in engine_state.hpp)
void h2d(void* dst, const void* src, size_t bytes, hipStream_t stream) {
  if (direct_copies()) { HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream)); HIP_CHECK(hipStreamSynchronize(stream)); return; }
  for (size_t off = 0; off < bytes; off += STAGE_CHUNK) {
    const size_t n = std::min(STAGE_CHUNK, bytes - off);
    void* st = staging().get(std::min(bytes, STAGE_CHUNK));
    std::memcpy(st, (const char*)src + off, n);
    HIP_CHECK(hipMemcpyAsync((char*)dst + off, st, n, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  staging().check();
}
void d2h(void* dst, const void* src, size_t bytes, hipStream_t stream) {
  if (direct_copies()) { HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream)); HIP_CHECK(hipStreamSynchronize(stream)); return; }
  for (size_t off = 0; off < bytes; off += STAGE_CHUNK) {
    const size_t n = std::min(STAGE_CHUNK, bytes - off);
    void* st = staging().get(std::min(bytes, STAGE_CHUNK));
    HIP_CHECK(hipMemcpyAsync(st, (const char*)src + off, n, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    staging().check();
    std::memcpy((char*)dst + off, st, n);
  }
}

namespace {

// a chain's tables on the device: its launches, ticket lists and dependency lists, n_done zeroed completion flags and the ticket
// counter.  Nothing half-built stays behind: on failure the buffers go with the local.
DevChain upload_chain(const std::vector<ChainLaunch>& lds, const std::vector<int32_t>& tk_launch, const std::vector<int32_t>& tk_block,
                      const std::vector<int32_t>& dep_off, const std::vector<int32_t>& dep, size_t n_done, hipStream_t stream) {
  DevChain dc;
  auto up = [&](auto& dst, const auto& v) {
    dst.alloc(std::max<size_t>(1, v.size()));
    if (!v.empty()) h2d(dst, v.data(), v.size() * sizeof(v[0]), stream);
  };
  up(dc.launches, lds); up(dc.tk_launch, tk_launch); up(dc.tk_block, tk_block); up(dc.dep_off, dep_off); up(dc.dep, dep);
  dc.tickets = (int32_t)tk_launch.size();
  n_done = std::max<size_t>(1, n_done);
  dc.done.alloc(n_done);
  dc.next.alloc(1);
  HIP_CHECK(hipMemsetAsync(dc.done, 0, n_done * sizeof(int32_t), stream));
  return dc;
}

// keep: refill d's buffers in place where they are large enough (the scratch schedule of lpmp_compute_pass_custom)
void upload_schedule(const Schedule& s, DevSchedule& d, hipStream_t stream, bool keep = false, bool adaptive_built = false) {
  if (keep) { d.graph.reset(); d.graph_primal.reset(); }
  else d.release();
  d.launches = s.launches; d.diff_tab_off = s.diff_tab_off; d.diff_tab = s.diff_tab; d.diff_tab_ne = s.diff_tab_ne; d.n_levels = s.n_levels; d.n_recv = s.n_recv; d.n_send = s.n_send; d.alg_bytes = s.alg_bytes;
  d.adaptive_built = adaptive_built;
  fill_device(d.recs, s.recs, stream);
  fill_device(d.ops, s.ops, stream);
  fill_device(d.packets, s.packets, stream);
  d.release_chain();
  if (!s.chains.empty() && !adaptive_built) {
    for (const ChainPlan& c : s.chains) {
      std::vector<ChainLaunch> lds;
      for (const auto& l : c.launches) lds.push_back({l.stride > 0 ? d.packets + l.pk_begin : nullptr, d.recs + l.rec_begin, d.ops, l.count, l.stride, l.flags});
      d.chains.push_back(upload_chain(lds, c.tk_launch, c.tk_block, c.dep_off, c.dep, c.tk_launch.size(), stream));
      DevChain& dc = d.chains.back();
      dc.kclass = c.kclass; dc.banded = c.banded; dc.level_loop = c.level_loop; dc.n_launches = (int32_t)c.launches.size();
      if (c.mailbox_rows > 0) {
        // a granule is valid when its tag is the epoch of the running launch: zeroed once, epochs start at 1
        const size_t bytes = (size_t)c.mailbox_rows * c.mailbox_width * 16;
        if (!dc.mailbox.try_alloc(bytes / sizeof(unsigned long long)))
          throw DeviceError("no device memory for the mailbox of a deep schedule (" + std::to_string(bytes >> 20) +
                            " MiB: 16 bytes per label and mailbox send); LPMP_NO_MAILBOX=1 plans the same schedule with completion flags only");
        HIP_CHECK(hipMemsetAsync(dc.mailbox, 0, bytes, stream));
      }
    }
    for (int32_t li : s.plain_launches) d.plain.push_back(s.launches[li]);
    HIP_CHECK(hipStreamSynchronize(stream));
    d.chain = true;
  }
}

// ... for an engine's model: counted (lpmp_schedules_built)
void upload_schedule(lpmp_engine* e, const Schedule& s, DevSchedule& d, bool keep = false, bool adaptive_built = false) {
  upload_schedule(s, d, e->stream, keep, adaptive_built);
  ++e->model.schedules_built;
}

void check_generic_limits(const Plan& p, const Schedule& s) {
  const int lim = GEN_MAXD;
  for (const auto& lr : s.launches) {
    if (lr.kclass != KC_GENERIC) continue;
    for (int64_t i = lr.begin; i < lr.end; ++i) {
      const UpdRec& r = s.recs[i];
      const int own = (r.kind_flags & 15) == LPMP_F_VECTOR ? r.d0 : r.d0 + r.d1;
      if (p.force_generic && r.n_send > GEN_ADAPTIVE_SENDS)
        throw UnsupportedError("adaptive sends: factor " + std::to_string(r.factor) + " has more active sends than the device kernel keeps improvements for");
      if (own > lim) throw UnsupportedError("factor " + std::to_string(r.factor) + ": dual size " + std::to_string(own) + " exceeds the device limit " + std::to_string(lim));
      for (int k = 0; k < r.n_recv + r.n_send; ++k)
        if (s.ops[r.op_begin + k].len > lim) throw UnsupportedError("message too long for the device kernels");
    }
  }
}

// one line, once per engine: a sweep of many dependent levels is latency-bound whatever executes it, and the order is the caller's
static void deep_schedule_note(lpmp_engine* e, int64_t n_levels, const char* what) {
  if (n_levels <= 64 || e->deep_note_given) return;
  e->deep_note_given = true;
  const char* q = std::getenv("LPMP_QUIET");
  if (q && q[0] == '1') return;
  std::fprintf(stderr, "lpmp: %s has %lld dependent levels (one launch step each): the factor order is the caller's input — "
               "lpmp_plan_suggest_order gives one with a level per colour (INTEGRATION.md 2a)\n", what, (long long)n_levels);
}

constexpr int64_t LAZY_SCHEDULES_MIN_FACTORS = (int64_t)1 << 20;
void ensure_device_schedules(lpmp_engine* e, int mode) {
  if (e->model.have_sched[mode]) return;
  for (int d = 0; d < 2; ++d) {
    plan_schedule(e->model.plan.get(), d, mode);
    deep_schedule_note(e, e->model.plan->sched_cache[d][mode].n_levels, d == 0 ? "the forward sweep" : "the backward sweep");
    check_generic_limits(e->model.plan->p, e->model.plan->sched_cache[d][mode]);
    upload_schedule(e, e->model.plan->sched_cache[d][mode], e->model.sched[d][mode]);
  }
  e->model.have_sched[mode] = true;
}

void ensure_pass_schedule(lpmp_engine* e, int mode) {
  if (e->model.have_pass[mode]) return;
  const bool timed_ = std::getenv("LPMP_PLAN_TIMES") != nullptr;
  auto t_last_ = std::chrono::steady_clock::now();
  auto lap_ = [&](const char* what) { if (!timed_) return; const auto now = std::chrono::steady_clock::now(); std::fprintf(stderr, "lpmp: pass schedule %-28s %.0f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last_).count()); t_last_ = now; };
  // (a three-level pass is the shape whose passes join: its own chain plan is only built if the joins do not check out)
  plan_pass_schedule(e->model.plan.get(), mode, false);
  deep_schedule_note(e, e->model.plan->pass_cache[mode].n_levels / 2, "a directional sweep");
  lap_("forward+backward planned");
  plan_rotation(e->model.plan.get(), mode);
  lap_("backward+forward planned, joins checked");
  if (!e->model.plan->rotation_ok[mode] && e->model.plan->pass_cache[mode].n_levels == 3) {
    e->model.plan->have_pass[mode] = false;
    plan_pass_schedule(e->model.plan.get(), mode, true);
    lap_("forward+backward planned again, with its chain plan");
  }
  check_generic_limits(e->model.plan->p, e->model.plan->pass_cache[mode]);
  upload_schedule(e, e->model.plan->pass_cache[mode], e->model.sched_pass[mode]);
  lap_("... uploaded");
  // LPMP_LAUNCH_LOG=<file> (profiling aid): one line per launch of the fused pass in execution order — level, class, records,
  // receives, sends, algorithmic bytes, packet stride — to lay beside the durations of a kernel trace (tools/launch_rates.py)
  if (const char* path = std::getenv("LPMP_LAUNCH_LOG")) {
    if (FILE* f = std::fopen(path, "w")) {
      std::fprintf(f, "level,kclass,records,receives,sends,bytes,stride\n");
      for (const auto& lr : e->model.plan->pass_cache[mode].launches)
        std::fprintf(f, "%d,%d,%lld,%lld,%lld,%lld,%d\n", lr.level, lr.kclass, (long long)(lr.end - lr.begin), (long long)lr.n_recv, (long long)lr.n_send, (long long)lr.bytes, lr.stride);
      std::fclose(f);
    }
  }
  e->model.rotation_ok[mode] = e->model.plan->rotation_ok[mode];
  if (e->model.rotation_ok[mode]) {
    upload_schedule(e, e->model.plan->bf_cache[mode], e->model.sched_bf[mode]);
    lap_("... uploaded");
    e->model.plan->rot[mode] = plan_rotation_chain(e->model.plan->pass_cache[mode], e->model.plan->bf_cache[mode], e->model.plan->p.nf);
    lap_("block relations of the steps");
    // the same with wide consume blocks, where a peer-minima launch can come (rotation_chain decides as here, mode by mode)
    e->model.rot_wide[mode] = RotationInfo();
    const RotationInfo& r0 = e->model.plan->rot[mode];
    if (e->pq_wide && e->use_peer_minima && r0.valid && r0.peer_minima && e->model.tab_flag == 0 && !e->model.rows &&
        (e->rot_opts.bands > 0 || (e->model.model_big && r0.t[1].bytes >= ((int64_t)64 << 20)))) {
      e->model.rot_wide[mode] = plan_rotation_chain(e->model.plan->pass_cache[mode], e->model.plan->bf_cache[mode], e->model.plan->p.nf, PQ_WIDE_RECORDS);
      lap_("... with wide consume blocks");
    }
    e->model.plan->bf_cache[mode] = Schedule();
  }
  // the host copy is only needed for its summary
  Schedule& h = e->model.plan->pass_cache[mode];
  h.recs.clear(); h.recs.shrink_to_fit(); h.ops.clear(); h.ops.shrink_to_fit(); h.packets.clear(); h.packets.shrink_to_fit();
  e->model.have_pass[mode] = true;
}

// ensure_pass_schedule plans a three-level pass whose consecutive passes join WITHOUT a chain plan of its own (the joined
// launch never reads it).  A pass that is then run on its own after all — another send rule, one pass at a time while the joined
// launch is unavailable — gets the plan the first time that happens: on an HBM-sized model the banded Infinity-Cache launch of
// the single pass.  The joined-launch templates of that mode point into the schedule's device arrays and are dropped (rebuilt on demand).
void ensure_pass_chain_plan(lpmp_engine* e, int mode) {
  if (e->model.pass_chain_tried[mode] || !e->use_chain || !e->use_blocked_passes) return;
  e->model.pass_chain_tried[mode] = true;
  const DevSchedule& d = e->model.sched_pass[mode];
  if (!e->model.have_pass[mode] || !e->model.rotation_ok[mode] || d.chain || d.n_levels != 3 || !e->model.model_big) return;
  e->model.plan->have_pass[mode] = false;
  plan_pass_schedule(e->model.plan.get(), mode, true);
  check_generic_limits(e->model.plan->p, e->model.plan->pass_cache[mode]);
  HIP_CHECK(hipStreamSynchronize(e->stream));
  e->model.release_rot_chains(mode);
  upload_schedule(e, e->model.plan->pass_cache[mode], e->model.sched_pass[mode]);
  Schedule& h = e->model.plan->pass_cache[mode];
  h.recs.clear(); h.recs.shrink_to_fit(); h.ops.clear(); h.ops.shrink_to_fit(); h.packets.clear(); h.packets.shrink_to_fit();
}

void issue_launches(lpmp_engine* e, const LaunchView& s, bool timed, hipStream_t stream, int only_level = 0) {
  for (const auto& lr : s.launches) {
    if (only_level > 0 && lr.level != only_level) continue;
    hipEvent_t a = nullptr, b = nullptr;
    if (timed) { a = e->get_event(); b = e->get_event(); HIP_CHECK(hipEventRecord(a, stream)); }
    // UpdateFactorPrimal always sends 'shared' (reference factors_messages.hxx:2357-2359), whatever the send rule
    const int rule = e->rtype == LPMP_RTYPE_RESIDUAL ? SWEEP_RESIDUAL : e->rtype == LPMP_RTYPE_ADAPTIVE ? SWEEP_ADAPTIVE : 0;
    const int flags = (e->primal_pass ? SWEEP_PRIMAL : rule) | e->model.nt_flag | e->model.tab_flag;
    // primal pass over pairwise factors that round themselves: those records take the generic kernels (ensure_primal)
    const bool pw_rounds = e->primal_pass && e->model.d_pw_unary && kc_is_pw(lr.kclass);
    if (pw_rounds)
      launch_sweep(KC_GENERIC, s.recs, s.ops, e->model.d_dual, e->model.d_const, e->model.d_tabs, e->model.d_lb, e->model.d_primal, e->model.d_pw_unary, lr.begin, lr.end - lr.begin, flags, stream);
    else if (kc_is_shared(lr.kclass)) {
      if (!launch_sweep_shared(lr.kclass, lr.stride > 0 ? s.packets + lr.pk_begin : nullptr, s.recs + lr.begin, s.ops, lr.stride, e->model.d_dual, e->model.d_const,
                               e->model.d_lb, e->model.d_primal, lr.end - lr.begin, flags, e->model.d_sh_desc, lr.sh_tab, lr.n_sh, stream))
        throw DeviceError("sweep: launch of shared class " + std::to_string(lr.kclass) + " without packets or tables");
    }
    else if (lr.kclass == KC_DIFF)     // (LDS by the launch's label counts, as the streaming class)
      launch_sweep_diff(lr.diff_band || lr.diff_shift_band, lr.diff_shift, s.recs, s.ops, e->model.d_dual, e->model.d_const, e->model.d_lb, e->model.d_primal, lr.begin, lr.end - lr.begin, flags | sweep_bigdim_flags(lr.max_dim), stream);
    else if (!(lr.stride != 0 &&
          launch_sweep_packed(lr.kclass, lr.stride > 0 ? s.packets + lr.pk_begin : nullptr, s.recs + lr.begin, s.ops, lr.stride, e->model.d_dual,
                              e->model.d_const, e->model.d_lb, e->model.d_primal, lr.end - lr.begin, flags, stream))) {
      // the packed classes have no op-by-op kernel: plan.cpp gives every launch of one packets or indirect records
      if (kc_is_packed(lr.kclass)) throw DeviceError("sweep: launch of packed class " + std::to_string(lr.kclass) + " without packets");
      launch_sweep(lr.kclass, s.recs, s.ops, e->model.d_dual, e->model.d_const, e->model.d_tabs, e->model.d_lb, e->model.d_primal, e->model.d_pw_unary, lr.begin, lr.end - lr.begin,
                   flags | (lr.kclass == KC_DENSE_BIG ? sweep_bigdim_flags(lr.max_dim) : 0), stream);   // (LDS of the streaming class: by the launch's label counts)
    }
    if (timed) {
      HIP_CHECK(hipEventRecord(b, stream));
      e->pending.push_back({a, b, lr.kclass, lr.end - lr.begin, lr.n_recv, lr.bytes, lr.kclass == KC_DIFF && lr.diff_band, lr.kclass == KC_DIFF && lr.diff_shift,
                            lr.kclass == KC_DIFF && lr.diff_shift && lr.diff_shift_band});
    }
  }
  HIP_CHECK(hipGetLastError());
}

// LPMP_CHAIN_TRACE=<file> (debugging): every chain run is followed by a synchronisation and its per-ticket time stamps
// (ticket in hand, predecessors seen, body done, published; 100 MHz) are written to the file together with the ticket
// -> launch map and the dependency lists: tools/chain_trace.py turns them into the latency budget of DESIGN.md 6
struct ChainTrace {
  DevBuf<long long> d; int32_t n = 0;
  // ("%p" in the path: this process's id — several ranks on one box)
  static const char* path() {
    static const std::string p = [] {
      const char* e = std::getenv("LPMP_CHAIN_TRACE");
      std::string s = e ? e : "";
      const size_t k = s.find("%p");
      if (k != std::string::npos) s.replace(k, 2, std::to_string((long long)getpid()));
      return s;
    }();
    return p.empty() ? nullptr : p.c_str();
  }
  long long* begin(int32_t n_tickets, hipStream_t s) {
    if (!path()) return nullptr;
    n = n_tickets;
    d.alloc((size_t)8 * n);
    HIP_CHECK(hipMemsetAsync(d, 0, (size_t)8 * n * sizeof(long long), s));
    return d;
  }
  template <class DC> void end(const DC& c, hipStream_t s, const int32_t* d_abort = nullptr) {
    if (!d) return;
    HIP_CHECK(hipStreamSynchronize(s));
    // the dump of a run in which a wait gave up is kept under its own name (later runs do not overwrite it)
    std::string out = path();
    if (d_abort) { int32_t a = 0; HIP_CHECK(hipMemcpy(&a, d_abort, sizeof(a), hipMemcpyDeviceToHost)); if (a) out += ".aborted"; }
    std::vector<long long> st((size_t)8 * n);
    std::vector<int32_t> tl((size_t)n), off((size_t)n + 1);
    HIP_CHECK(hipMemcpy(st.data(), d, st.size() * sizeof(long long), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(tl.data(), c.tk_launch, tl.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(off.data(), c.dep_off, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int32_t> dep((size_t)off[n]);
    if (!dep.empty()) HIP_CHECK(hipMemcpy(dep.data(), c.dep, dep.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    d.reset();
    if (FILE* f = std::fopen(out.c_str(), "wb")) {
      const int64_t hdr[2] = {n, off[n]};
      std::fwrite(hdr, sizeof(hdr), 1, f);
      std::fwrite(st.data(), sizeof(long long), st.size(), f);
      std::fwrite(tl.data(), sizeof(int32_t), tl.size(), f);
      std::fwrite(off.data(), sizeof(int32_t), off.size(), f);
      std::fwrite(dep.data(), sizeof(int32_t), dep.size(), f);
      std::fclose(f);
    }
  }
};

// the abort words of the chain executor: allocated and zeroed the first time a chain runs
void ensure_chain_abort(lpmp_engine* e) {
  if (e->d_chain_abort) return;
  e->d_chain_abort.alloc(CHAIN_ABORT_WORDS);
  HIP_CHECK(hipMemsetAsync(e->d_chain_abort, 0, CHAIN_ABORT_WORDS * sizeof(int32_t), e->stream));
}
// the arguments every chain launch has: the chain's arrays, the abort words, the next epoch, the bound of a wait, the trace
// (everything else zero: no bound rows, no mailbox, plain ticket lists)
ChainArgs chain_args(lpmp_engine* e, DevChain& c, int32_t n_tickets, long long* trace) {
  ChainArgs ca{};
  ca.dep_off = c.dep_off; ca.dep = c.dep; ca.done = c.done; ca.next = c.next; ca.abort_flag = e->d_chain_abort;
  ca.tk_launch = c.tk_launch; ca.tk_block = c.tk_block; ca.n_tickets = n_tickets; ca.epoch = ++c.epoch;
  ca.trace = trace; ca.timeout_ticks = chain_timeout_ticks();
  return ca;
}

// one sweep over a device schedule; long launch chains (row-major grids: one launch per anti-diagonal)
// are captured once into a hipGraph and replayed
void run_schedule(lpmp_engine* e, DevSchedule& s) {
  if (s.launches.empty()) return;
  if (e->timing) { issue_launches(e, s.view(), true, e->stream); if (e->pending.size() > 4096) e->drain_timing(); return; }
  // (a primal pass rounds inside the packed kernels' chain form too; the generic chain kernels carry no labels, and
  // pairwise factors that round themselves need the generic kernels: those passes stay launch by launch)
  bool chain_ok = s.chain && e->use_chain;
  if (chain_ok && e->primal_pass) {
    if (e->model.d_pw_unary) chain_ok = false;
    for (const auto& c : s.chains) if (kc_width(c.kclass) == 0) chain_ok = false;
  }
  if (chain_ok) {
    ensure_chain_abort(e);
    // UpdateFactorPrimal always sends 'shared' (issue_launches)
    const int rule = e->primal_pass ? SWEEP_PRIMAL : e->rtype == LPMP_RTYPE_RESIDUAL ? SWEEP_RESIDUAL : e->rtype == LPMP_RTYPE_ADAPTIVE ? SWEEP_ADAPTIVE : 0;
    // classes are independent of each other (chain_plan.cpp): the plain launches first, then one persistent launch per class
    if (!s.plain.empty()) issue_launches(e, s.plain_view(), false, e->stream);
    for (auto& c : s.chains) {
      if (c.level_loop) {
        // LPMP_LEVEL_TRACE=<file> (debugging): time stamps of the first LEVEL_TRACE_MAX levels, written after a synchronisation
        static const char* lt_path = std::getenv("LPMP_LEVEL_TRACE");
        DevBuf<long long> d_lt;
        const size_t lt_n = 8 + 8 * LEVEL_TRACE_MAX;
        if (lt_path) { d_lt.alloc(lt_n); HIP_CHECK(hipMemset(d_lt, 0, lt_n * sizeof(long long))); debug_set_level_trace(d_lt); }
        if (!launch_level_loop(c.kclass, rule | e->model.tab_flag, c.launches, c.n_launches, e->model.d_dual, e->model.d_const, e->model.d_tabs, e->model.d_lb, e->stream))
          throw DeviceError("level loop: no kernel for class " + std::to_string(c.kclass));
        if (lt_path) {
          HIP_CHECK(hipStreamSynchronize(e->stream));
          std::vector<long long> h(lt_n);
          HIP_CHECK(hipMemcpy(h.data(), d_lt, lt_n * sizeof(long long), hipMemcpyDeviceToHost));
          debug_set_level_trace(nullptr);
          if (FILE* f = std::fopen(lt_path, "wb")) { std::fwrite(h.data(), sizeof(long long), h.size(), f); std::fclose(f); }
        }
        continue;
      }
      HIP_CHECK(hipMemsetAsync(c.next, 0, sizeof(int32_t), e->stream));
      ChainTrace tr;
      ChainArgs ca = chain_args(e, c, c.tickets, tr.begin(c.tickets, e->stream));
      ca.mailbox = c.mailbox;
      if (!launch_chain(c.kclass, rule | (c.banded ? 0 : e->model.nt_flag) | e->model.tab_flag, ca, c.launches, e->model.d_dual, e->model.d_const, e->model.d_tabs, e->model.d_lb, e->model.d_primal, e->stream,
                        nullptr, 1, false, 2, false, ChainAhead(), e->chain_max_wgs))
        throw DeviceError("chain executor: no kernel for class " + std::to_string(c.kclass));
      tr.end(c, e->stream, e->d_chain_abort);
    }
    HIP_CHECK(hipGetLastError());
    e->chain_ran = true;
    return;
  }
  // (graphs of up to ~20 k kernel nodes were exercised — C5; beyond 200 k the nodes are issued one by
  // one instead of instantiating a graph of that size)
  if (e->use_graph && s.launches.size() > 8 && s.launches.size() <= 200000) {
    hipGraphExec_t& exec = e->primal_pass ? s.graph_primal.g : s.graph.g;
    if (!exec) {
      hipGraph_t g = nullptr;
      if (!e->capture_stream) e->capture_stream = stream_pool().take(e->device);
      HIP_CHECK(hipStreamBeginCapture(e->capture_stream, hipStreamCaptureModeThreadLocal));
      try { issue_launches(e, s.view(), false, e->capture_stream); }
      catch (...) { (void)hipStreamEndCapture(e->capture_stream, &g); if (g) (void)hipGraphDestroy(g); throw; }
      HIP_CHECK(hipStreamEndCapture(e->capture_stream, &g));
      HIP_CHECK(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
      HIP_CHECK(hipGraphDestroy(g));
    }
    HIP_CHECK(hipGraphLaunch(exec, e->stream));
    return;
  }
  issue_launches(e, s.view(), false, e->stream);
}

// weight / receive-mask rows of an iterator-range pass as they come over the C ABI: offsets start at 0 and do not
// decrease, and a row with entries needs the array it indexes
void check_rows(int64_t n, const int64_t* om_off, const double* om, const int64_t* mk_off, const uint8_t* mk) {
  if (n <= 0) return;
  if (om_off[0] != 0 || mk_off[0] != 0) throw std::runtime_error("omega / receive-mask offsets must start at 0");
  for (int64_t i = 0; i < n; ++i)
    if (om_off[i + 1] < om_off[i] || mk_off[i + 1] < mk_off[i]) throw std::runtime_error("omega / receive-mask offsets must not decrease");
  if (!om && om_off[n] > 0) throw std::runtime_error("omega array missing");
  if (!mk && mk_off[n] > 0) throw std::runtime_error("receive-mask array missing");
}

// n joined passes (H, W, (K, W)^(n-1), T) as ONE persistent launch of the chain executor.  Tickets are not taken step by
// step but in a skewed order: inside a group of `depth` consecutive steps, band j of the group's d-th step comes at time
// j + lag * d, so that the pairwise tables a step reads are read again by the next step while they are still in the
// 256 MiB Infinity Cache (every table is needed by both of its endpoints, i.e. by consecutive steps).  Only the order
// changes: the dependency flags keep every result identical to the sequential sweeps.  Returns nullptr when the model
// does not qualify (then the steps run as one launch each).
// Calls of n > ROT_EXPLICIT_MAX passes use a PERIODIC template instead of explicit lists: with `depth` even the groups of
// `depth` steps from the second one on are all alike — K, W, K, W with the same bands in the same order, their dependencies
// the same offsets into themselves and into the group before — so the lists of a template call (prologue = the first two
// groups, ONE more group = the period, then the tail: T, or K W T for an odd pass count) describe every pass count of that
// parity: the kernel maps ticket t to (template ticket, copy of the period) (kernels.hip, chain_ticket_ref), and the
// completion flags are a ring of a few groups.  Host work, upload and device memory of an n-pass launch no longer depend on n.
constexpr int ROT_EXPLICIT_MAX = 7;
// (the window (bands, lag, depth) follows the model: order.cpp rot_geometry; the tiled order: order.cpp make_tiles / tiled_order)
RotChain* rotation_chain(lpmp_engine* e, int mode, int n_call) {
  // The peer-minima form is decided first, because the wide consume form has block relations of its own and everything below is
  // sized by block counts: the structure allows it (order.cpp), the tables are doubles in the packed layout (and, further down, the
  // buffer can be had).  Every other launch is planned from the plan's own relations, as ever.
  const RotationInfo& ri_own = e->model.plan->rot[mode];
  const char* pq_why = !e->use_peer_minima ? "switched off (LPMP_NO_PEER_MINIMA)" : !ri_own.peer_minima ? ri_own.peer_minima_why.c_str()
                     : e->model.tab_flag != 0 ? "float tables" : e->model.rows ? "rows layout" : nullptr;
  const bool wide = !pq_why && e->pq_wide && e->model.rot_wide[mode].valid;
  const RotationInfo& ri = wide ? e->model.rot_wide[mode] : ri_own;
  RotOrder& ro = e->model.rot_order[mode][wide ? 1 : 0];
  if (!ro.have_geo) { ro.geo = rot_geometry(e->rot_opts, ri); ro.have_geo = true; }
  const RotGeometry& geo = ro.geo;
  const int rot_bands = e->rot_opts.bands;
  // Band order or tiled order?  Measured (profiles/r06_tile_sweep.txt, r06_blocked_pass_probe_tiles_*.txt; tiles of 1024 blocks): where
  // the band order runs at depth 4 it is as good or better (1024^2: 5.09 against 5.31 ms per pass, 2048^2: 21.35 / 21.26); where
  // the reach of the dependencies has pushed it to depth 2 or out of the cache, tiles win — 3072^2: 49.5 -> 47.7 ms, 256 x 4096: 5.89
  // -> 5.44, 128 x 8192 (no band order fits: 6.95 launch by launch) -> 5.37, 3-D grids 96^3 x 32 labels: 8.88 -> 7.27, 128^3 x 16
  // labels: 6.23 -> 5.72.  Calls of fewer than 4 passes keep the band order (single passes: 9.0 against 6.8 ms at 1024^2).
  // Depth of the tiled order (TileSet::depth): the flat tiles of a 2-D grid lose about 4 % per step: depth 8; the balls of a 3-D grid
  // 16 %: depth 4 — measured there: depth 2 / 4 / 6 / 8 = 7.9 / 7.27 / 7.28 / 7.6 ms per pass at 96^3 x 32 labels, 5.92 / 5.72 / - /
  // 7.24 at 128^3 x 16).
  // Peer-minima launches (EXPERIMENTS.md T): K / T read no table, so the only second reader of a table is the W step of the next
  // pass, and the band order can serve at most every second of those reads on-die, at a distance the reach of a grid row keeps at
  // the edge of the cache.  They take a geometry of their own for calls of at least 12 passes where a W step's tables exceed the
  // Infinity Cache: large tiles (few delayed blocks), groups of 8 steps, and the skew of the band order over the sub-bands of the
  // tiles (order.cpp skewed_tile_order), whose lag has to cover a row of a tile only.  LPMP_PQ_TILES=0 returns them to the rule of
  // every other launch; LPMP_PQ_TILES=T / LPMP_PQ_SUB / LPMP_PQ_SUBLAG / LPMP_PQ_SUBGAP force tile blocks, sub-bands per tile, their
  // lag and the gap behind a predecessor.  Tiles forced with LPMP_ROT_TILES take the sub-bands their size gives (none when small).
  JoinedOrder ord{geo.bands, geo.lag, geo.depth, nullptr};
  PqGeometry pqg;
  TileSet* tiles = nullptr;
  {
    const bool worthwhile = ri.valid && kc_is_dense(ri.kclass) && !kc_is_var(ri.kclass) &&
                            (rot_bands > 0 || (e->model.model_big && ri.t[1].bytes >= ((int64_t)64 << 20)));
    const bool tileable = worthwhile && ri.t[0].nb == ri.t[2].nb && ri.t[3].nb == ri.t[2].nb;
    // (with LPMP_PQ_TILES=T the rule also runs under a forced band count: that is how a model of test size reaches it)
    // Calls of fewer than PQ_MIN_PASSES passes keep the old order: a 5-pass call was 3 % slower in the new one (20.41 against 19.74 ms
    // in the kernel trace; its T tickets wait 22 instead of 12 us) — 11 steps are one group of 8 and a rest; from 12 passes on every
    // call is a periodic template.  6 to 11 passes were not measured.  LPMP_PQ_MIN_PASSES moves the threshold (tests, probes).
    bool pq_own = tileable && !pq_why && e->pq_tiles != 0 && !e->rot_tiles_set && (rot_bands <= 0 || e->pq_tiles > 0) && n_call >= e->pq_min_passes;
    if (pq_own) {
      if (!ro.have_pq_geo) { ro.pq_geo = peer_minima_geometry(ri, e->pq_tiles > 0 ? e->pq_tiles : 0); ro.have_pq_geo = true; }
      pq_own = ro.pq_geo.use || e->pq_tiles > 0;
    }
    // (the buffer of the minima first: without it the launch is not a peer-minima launch and keeps its old order)
    if (pq_own && !e->model.d_peerq.get() && !e->model.d_peerq.try_alloc((size_t)e->model.plan->p.nf * 32)) pq_own = false;
    const int want = !tileable ? 0
                   : pq_own ? ro.pq_geo.tile_blocks
                   : e->rot_tiles_set ? e->rot_tiles
                   : (rot_bands <= 0 && (geo.depth != 4 || !geo.fits) && n_call >= 4 ? 1024 : 0);
    if (want > 0) {
      TileSet& ts = ro.tile_sets[want];
      if (ts.T != want) ts = make_tiles(ri, want);
      ord.tiles = tiles = &ts;
      if (!e->rot_opts.depth_set) ord.depth = ts.depth;
      // the skew over the tiles: the rule's own tiles, and tiles forced with LPMP_ROT_TILES on a peer-minima launch where they are large
      // enough for two sub-bands (tiles the old rule chose stay plain)
      if (!pq_why && e->pq_tiles != 0 && (pq_own || e->rot_tiles_set)) {
        pqg = pq_own ? ro.pq_geo : peer_minima_geometry(ri, want);
        if (e->pq_sub > 0) pqg.sub = e->pq_sub;
        if (e->pq_sublag > 0) pqg.sub_lag = e->pq_sublag;
        if (e->pq_subgap >= 0) pqg.sub_gap = e->pq_subgap;
        ord.sub = pqg.sub; ord.sub_lag = pqg.sub_lag; ord.sub_gap = pqg.sub_gap;
      }
    }
  }
  const int depth = ord.depth;
  // template: groups 0, 1 (prologue), 2 (the period) and a tail as long as the call's: r = (2 n + 1) mod depth steps
  const int tail = depth % 2 == 0 ? (2 * n_call + 1) % depth : 0;
  const int n_template = (3 * depth + tail - 1) / 2;
  const bool periodic = depth % 2 == 0 && n_call > ROT_EXPLICIT_MAX && n_call >= n_template && !std::getenv("LPMP_ROT_EXPLICIT");
  const int n = periodic ? n_template : n_call;
  // (a periodic template serves every call of its tail, depth and order: short and long calls of one model may differ in the last two)
  const int key = periodic ? -(tail + 32 * depth + (ord.tiles ? 1024 : 0) + (ord.sub > 1 ? 2048 : 0)) : n_call;
  auto it = e->model.rot_chain[mode].find(key);
  if (it != e->model.rot_chain[mode].end()) { it->second.last_use = ++e->rot_clock; return it->second.n_steps > 0 ? &it->second : nullptr; }
  RotChain& rc = e->model.rot_chain[mode][key];           // n_steps == 0: tried, not possible
  rc.last_use = ++e->rot_clock;
  const bool verbose = std::getenv("LPMP_ROT_VERBOSE") != nullptr;
  const auto t_begin = std::chrono::steady_clock::now();
  auto no = [&](const char* why) -> RotChain* { if (verbose) std::fprintf(stderr, "lpmp: %d passes stay one launch per step: %s\n", n_call, why); return nullptr; };
  if (!ri.valid) return no("the pass does not have the H, W, K, T shape of one packed class");
  // a model whose tables fit the caches gains nothing from the order and is launch-bound: one launch per step then
  // (nor does one that fits the Infinity Cache as a whole: plain launches already re-read it on-die, and the chain's
  // agent-scope accesses only cost — C2, 512 x 512 8-label Potts: 0.065 ms per pass as launches, 0.10 as a chain)
  if (rot_bands <= 0 && (ri.t[1].bytes < ((int64_t)64 << 20) || !e->model.model_big)) return no("the model fits the caches");
  // (the run-time-dims classes read their tables with 8-byte loads of rows that are not line-aligned: as a chain in
  // Infinity-Cache order 1024 x 1024 x 21 labels takes 5.48 ms per pass against 4.38 launch by launch)
  if (rot_bands <= 0 && kc_is_var(ri.kclass)) return no("run-time-dims class");
  // (Potts steps stream message vectors only, at 7.6 TB/s with the non-temporal policy; as a chain their agent-scope
  // vector loads make 2048 x 2048 x 32 labels 6.4 ms per pass against 3.2)
  if (rot_bands <= 0 && !kc_is_dense(ri.kclass)) return no("no pairwise tables to re-read (Potts)");
  // bands: about 16 MiB of algorithmic bytes per band of a step.  What a group keeps alive between two reads of a table is
  // lag * depth bands (3 * 4 * 16 MiB = 192 MiB of the 256 MiB Infinity Cache); measured on C3: windows of 200-230 MB are
  // the fastest whatever the split (1024:3:4 5.09, 2048:4:6 5.03, 1536:3:6 5.09 ms per pass), 290 MB and more lose the
  // reuse (1024:3:5 5.67, 1024:3:6 6.37), lag 2 leaves the waiting workgroups less slack (1024:2:4 5.24)
  // (round 6: lag and depth follow the reach of the dependencies — order.cpp rot_geometry; C3 keeps 3 and 4)
  if (!geo.fits && !ord.tiles) return no("a step's dependencies reach further than the Infinity Cache window can cover");
  if (ord.tiles && verbose) std::fprintf(stderr, "lpmp:   %d tiles of about %d blocks per step, radius %.1f hops, delayed after 1 / 3 / 5 / 7 steps: %.2f / %.2f / %.2f / %.2f\n", tiles->n, tiles->T,
                                         tiles->radius, tiles->delayed[1], tiles->delayed[3], tiles->delayed[5], tiles->delayed[7]);
  if (ord.tiles && ord.sub > 1 && verbose) {
    extend_tile_delays(ri, *tiles);          // (steps 8 to 15: only this line shows them)
    std::fprintf(stderr, "lpmp:   peer-minima geometry: tiles of %.0f MiB of a W step (%.0f W blocks; steps move %.2f / %.2f / %.2f / %.2f GB), depth %d, %d sub-bands per tile at lag %d, gap %d, "
                 "delayed after 7 / 11 / 15 steps: %.2f / %.2f / %.2f; predicted HBM share of the table reads %.2f\n", pqg.tile_bytes / 1048576.0, pqg.w_blocks_per_tile,
                 pqg.step_bytes[0] / 1e9, pqg.step_bytes[1] / 1e9, pqg.step_bytes[2] / 1e9, pqg.step_bytes[3] / 1e9, ord.depth, ord.sub, ord.sub_lag, ord.sub_gap,
                 tiles->delayed[7], tiles->delayed[11], tiles->delayed[15], peer_minima_hbm_share(*tiles, ord.depth));
  }
  if (!pq_why && !e->model.d_peerq.get() && !e->model.d_peerq.try_alloc((size_t)e->model.plan->p.nf * 32)) {
    if (wide) {   // the old form then, planned from its own relations: this entry goes, the wide relations with it
      e->model.rot_chain[mode].erase(key);
      e->model.rot_wide[mode] = RotationInfo();
      return rotation_chain(e, mode, n_call);
    }
    pq_why = "no device memory for the published minima";
    ord.sub = 1;
  }
  JoinedTables jt;
  const std::string why = joined_pass_tables(ri, ord, n, periodic, jt, verbose ? stderr : nullptr);
  if (!why.empty()) return no(why.c_str());
  if (periodic && (int64_t)48 * (int64_t)(2 * jt.per_len) / jt.ring + 64 >= (1 << CHAIN_GEN_BITS)) throw std::runtime_error("rotation chain: ring too small for its generation counter");
  const int n_steps = 2 * n + 1;
  const bool pq = pq_why == nullptr;
  if (verbose) std::fprintf(stderr, "lpmp:   peer minima: %s\n", pq ? "W publishes, K / T read no table" : pq_why);
  std::vector<ChainLaunch> lds;
  for (int s = 0; s < n_steps; ++s) {
    const auto& t = ri.t[jt.step_tmpl[s]];
    const DevSchedule& ds = t.sched == 0 ? e->model.sched_pass[mode] : e->model.sched_bf[mode];
    const int32_t row = jt.step_row[s];
    int32_t hist = row < 0 ? 0 : (jt.step_tmpl[s] == 1 ? HIST_END : HIST_MID) | (row << 2);
    if (pq) hist |= jt.step_tmpl[s] == 1 ? CHAIN_LAUNCH_PQ_PUBLISH : CHAIN_LAUNCH_PQ_CONSUME;
    lds.push_back({t.lr.stride > 0 ? ds.packets + t.lr.pk_begin : nullptr, ds.recs + t.lr.begin, ds.ops, t.lr.end - t.lr.begin, t.lr.stride, hist});
    rc.factors += t.factors; rc.recv += t.recv; rc.bytes += t.bytes;
    if (periodic && s >= 2 * depth && s < 3 * depth) { rc.per_factors += t.factors; rc.per_recv += t.recv; rc.per_bytes += t.bytes; }
  }
  // (periodic: the kernel looks a ticket's launch up at its TEMPLATE step — the steps of a later copy of the period are the
  // same K / W launches, and the tail's the same K, W, T; only the bound row in `pad` moves with the copy, depth / 2 rows
  // per copy — so this table, too, is the template's whatever the call's pass count)
  const int64_t N = (int64_t)jt.tk_launch.size();
  const size_t n_done = periodic ? (size_t)jt.ring : (size_t)N;
  rc.dev_bytes = lds.size() * sizeof(ChainLaunch) + (jt.tk_launch.size() + jt.tk_block.size() + jt.dep_off.size() + jt.dep.size() + n_done + 1) * sizeof(int32_t);
  // tickets ahead: the shipped peer-minima form only, and only while the launch table fits the kernel's LDS copy.  The descriptors
  // are device bytes of the cached chain like its other arrays, counted before the cache makes room; a chain that fits the cache's
  // bound only without them is built plain
  int ahead = pq && e->pq_ahead != 0 && pq_ahead_applies(e->pq_lds, e->pq_hold, wide, e->pq_scatter, (int)lds.size()) ? e->pq_ahead : 0;
  const size_t desc_bytes = (size_t)N * TICKET_DESC_WORDS * sizeof(int32_t);
  if (ahead && rc.dev_bytes <= e->rot_cache_limit && rc.dev_bytes + desc_bytes > e->rot_cache_limit) ahead = 0;
  if (ahead) rc.dev_bytes += desc_bytes;
  // bound the cache in bytes: drop the least recently used built chains (of any mode) until the new one fits; the stream is drained first
  for (bool drained = false; e->model.rot_cache_bytes + rc.dev_bytes > e->rot_cache_limit;) {
    std::map<int, RotChain>* vm = nullptr; std::map<int, RotChain>::iterator victim;
    for (auto& m : e->model.rot_chain)
      for (auto i2 = m.begin(); i2 != m.end(); ++i2)
        if (i2->second.n_steps > 0 && (!vm || i2->second.last_use < victim->second.last_use)) { vm = &m; victim = i2; }
    if (!vm) break;
    if (!drained) { HIP_CHECK(hipStreamSynchronize(e->stream)); drained = true; }
    e->model.rot_cache_bytes -= std::min(e->model.rot_cache_bytes, victim->second.dev_bytes);
    vm->erase(victim);
  }
  std::vector<int32_t> desc;
  if (ahead) desc = ticket_descriptors(jt.tk_launch, jt.tk_block, jt.dep_off, jt.dep, e->pq_desc_inline);
  try {
    rc.dc = upload_chain(lds, jt.tk_launch, jt.tk_block, jt.dep_off, jt.dep, n_done, e->stream);
    if (ahead) {
      rc.dc.desc.alloc(std::max<size_t>(1, desc.size()));
      if (!desc.empty()) h2d(rc.dc.desc, desc.data(), desc.size() * sizeof(int32_t), e->stream);
      rc.dc.desc_inline = e->pq_desc_inline;
    }
    rc.dc.n_launches = (int32_t)lds.size();
    HIP_CHECK(hipStreamSynchronize(e->stream));
  } catch (...) {
    // nothing half-built stays behind: the entry goes (a later call tries again), the bytes were never counted
    e->model.rot_chain[mode].erase(key);
    throw;
  }
  rc.dc.kclass = ri.kclass;
  e->model.rot_cache_bytes += rc.dev_bytes;
  ++e->model.schedules_built;
  rc.peer_minima = pq; rc.pq_wide = pq && wide; rc.pq_ahead = ahead;
  rc.n_steps = n_steps; rc.periodic = periodic; rc.n_tmpl = n; rc.depth = depth; rc.ring = jt.ring; rc.per_begin = jt.per_begin; rc.per_len = jt.per_len;
  if (verbose && pq) {
    int per_cu = 0;
    int num_regs = 0, scratch = 0;
    const bool three = e->pq_lds != 0 && e->pq_hold == 3;
    const unsigned grid = chain_pq_grid(e->pq_lds, e->pq_hold, rc.pq_wide, e->pq_scatter, (int)std::min<int64_t>(N, INT32_MAX), &per_cu, &num_regs, &scratch, ahead, e->chain_max_wgs);
    std::fprintf(stderr, "lpmp:   peer minima launch (LPMP_PQ_LDS=%d, LPMP_PQ_WIDE=%d: %d records per consume ticket, %lld tickets): %d resident workgroups per CU, grid %u; "
                 "%d tables in registers, %d registers, %d bytes of scratch; publish: %s\n",
                 e->pq_lds, rc.pq_wide ? 1 : 0, ri.consume_gpb, (long long)N, per_cu, grid, three ? 3 : 2, num_regs, scratch, three && e->pq_scatter ? "reduce-scatter" : "all-reduce");
    // (a line of its own: the line above is matched to its end by tests that were written before this form existed)
    std::fprintf(stderr, "lpmp:   peer minima launch; tickets: %s\n", ahead ? "ahead (a descriptor per ticket, the launch table in LDS)" : "plain");
    // dependencies per ticket, and what the descriptors' inline part covers
    const std::vector<int64_t> h = ticket_dep_histogram(jt.dep_off, TICKET_DESC_INLINE + 1);
    std::string hs; int64_t in = 0;
    for (size_t c = 0; c < h.size(); ++c) { hs += (c ? " " : "") + std::to_string(h[c]); if ((int)c <= e->pq_desc_inline) in += h[c]; }
    std::fprintf(stderr, "lpmp:   dependencies per ticket (0 ... %d, more): %s; %.4f of the tickets within an inline cap of %d\n", TICKET_DESC_INLINE, hs.c_str(),
                 N > 0 ? (double)in / (double)N : 1.0, e->pq_desc_inline);
  }
  if (verbose)
    std::fprintf(stderr, "lpmp: %d passes as one launch%s: %lld tickets, %d bands, lag %d, depth %d (reach %.1f MB of %.1f MB per band); built and uploaded in %.0f ms\n", n,
                 periodic ? (ord.tiles ? (jt.sub > 1 ? " (periodic template, skewed tiled order)" : " (periodic template, tiled order)") : " (periodic template)")
                          : ord.tiles ? (jt.sub > 1 ? " (skewed tiled order)" : " (tiled order)") : "", (long long)N, ord.bands, jt.lag, depth,
                 geo.reach_bytes / 1e6, (double)ri.t[1].bytes / ord.bands / 1e6, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  return &rc;
}

bool run_rotation_chain(lpmp_engine* e, int mode, int n, double* lb_hist = nullptr) {
  if (!e->use_chain || !e->use_blocked_passes || e->primal_pass || e->rtype != LPMP_RTYPE_SHARED) return false;
  RotChain* rc = rotation_chain(e, mode, n);
  if (!rc) return false;
  ensure_chain_abort(e);
  auto& c = rc->dc;
  HIP_CHECK(hipMemsetAsync(c.next, 0, sizeof(int32_t), e->stream));
  // periodic template: the period runs once in the template and `extra` more times in this call
  const int extra = rc->periodic ? (n - rc->n_tmpl) / (rc->depth / 2) : 0;
  if (rc->periodic && (extra < 0 || rc->n_tmpl + extra * (rc->depth / 2) != n)) throw std::runtime_error("rotation chain: pass count does not fit the template");
  if (rc->periodic && c.epoch >= (1 << (31 - CHAIN_GEN_BITS)) - 2) {   // the epoch shares the flag word with the generation: start over
    HIP_CHECK(hipMemsetAsync(c.done, 0, (size_t)rc->ring * sizeof(int32_t), e->stream));
    c.epoch = 0;
  }
  ChainTrace tr;
  const int32_t n_tickets = c.tickets + extra * rc->per_len;
  ChainArgs ca = chain_args(e, c, n_tickets, rc->periodic ? nullptr : tr.begin(c.tickets, e->stream));
  if (lb_hist) { ca.lb_hist = lb_hist; ca.hist_stride = e->model.plan->p.nf; ca.hist_rows = n - 1; }
  ChainAhead ahead;
  if (rc->pq_ahead) { ahead.desc = c.desc; ahead.desc_inline = c.desc_inline; ahead.n_launches = c.n_launches; ahead.form = rc->pq_ahead; }
  if (rc->periodic) { ca.per_begin = rc->per_begin; ca.per_len = rc->per_len; ca.per_count = 1 + extra; ca.per_row_shift = rc->depth / 2; ca.ring = rc->ring; }
  hipEvent_t a = nullptr, b = nullptr;
  if (e->timing) { a = e->get_event(); b = e->get_event(); HIP_CHECK(hipEventRecord(a, e->stream)); }
  // (plain table loads, not the streaming policy: the second reader of a table is meant to find it in the Infinity Cache)
  if (rc->peer_minima && !e->model.d_peerq.get()) throw std::runtime_error("rotation chain: the buffer of the published minima is gone");
  if (!launch_chain(c.kclass, e->model.tab_flag, ca, c.launches, e->model.d_dual, e->model.d_const, e->model.d_tabs, e->model.d_lb, nullptr, e->stream, rc->peer_minima ? e->model.d_peerq.get() : nullptr, e->pq_lds, rc->pq_wide, e->pq_hold, e->pq_scatter, ahead, e->chain_max_wgs)) throw DeviceError("chain executor: no kernel for class " + std::to_string(c.kclass));
  if (!rc->periodic) tr.end(c, e->stream, e->d_chain_abort);
  if (e->timing) {
    HIP_CHECK(hipEventRecord(b, e->stream));
    e->pending.push_back({a, b, c.kclass, rc->factors + extra * rc->per_factors, rc->recv + extra * rc->per_recv, rc->bytes + extra * rc->per_bytes});
    e->ct[c.kclass].chain_launches++;
  }
  if (rc->peer_minima) e->ct[c.kclass].peer_minima_launches++;   // (counted with timing off, too: passes that run ahead are never timed)
  HIP_CHECK(hipGetLastError());
  e->chain_ran = true;
  return true;
}

void require_model(const lpmp_engine* e) { if (!e || !e->model.plan) throw StateError("no model uploaded"); }
void require_mode(const lpmp_engine* e) {
  require_model(e);
  if (e->model.mode < 0) throw StateError("no reparametrization mode set");   // reference LP_MP.h:414,458
}

}  // namespace

// (settle, check_chain: defined below, declared in engine_state.hpp like rows_refresh and require_consts)
// rows layout: bring the side that is about to be read up to date (stream-ordered copies of the message vectors)
void rows_refresh(lpmp_engine* e) {   // packed duals -> rows, before anything computes on the rows
  // (every hand-over first writes the rows out — rows_flush — and only then lets the caller write: both copies newer than the
  // other would mean one of the two gets lost)
  if (e->model.rows && e->model.rows_stale && e->model.packed_stale) throw StateError("rows layout: packed duals and rows both hold newer vectors");
  if (e->model.rows && e->model.rows_stale) { launch_rows_copy(e->model.d_rowrecs, e->model.n_rowrecs, e->model.d_const, e->model.d_dual, e->model.d_rows, 1, e->stream); HIP_CHECK(hipGetLastError()); e->model.rows_stale = false; }
}
static void rows_flush(lpmp_engine* e) {     // rows -> packed duals, before the packed array is handed to anybody
  if (e->model.rows && e->model.packed_stale) { launch_rows_copy(e->model.d_rowrecs, e->model.n_rowrecs, e->model.d_const, e->model.d_dual, e->model.d_rows, 2, e->stream); HIP_CHECK(hipGetLastError()); e->model.packed_stale = false; }
}
// the constants are unspecified after a refused lpmp_upload_costs: whatever would read them says so — passes, bounds, the primal
// cost.  The lpmp_boundary_* / lpmp_halo_* kernels (boundary.hip) touch duals only and are not checked.
void require_consts(const lpmp_engine* e) {
  if (e->model.const_bad) throw StateError("the constants are unspecified since lpmp_upload_costs refused them: upload costs the table precision accepts, or the model");
}
static void begin_compute(lpmp_engine* e) { require_consts(e); rows_refresh(e); if (e->model.rows) e->model.packed_stale = true; }

namespace {
// The listed rows of lpmp_set_vectors / lpmp_set_constants.  Validates the list (range, kind: `vectors` says which kind the call
// takes and wrong_kind how it refuses the other, no factor twice), lets `fill(i, f, src_row)` make record i, checks the stride
// against the longest row, settles the engine, uploads the records into d_recs and packs a host source row after row into
// d_setsrc.  Returns the device source and its stride, {nullptr, 0} for an empty list.
struct ListedSrc { const double* src; int64_t stride; };
template <class Rec, class Fill>
ListedSrc listed_rows(lpmp_engine* e, const std::string& who, int64_t n, const int32_t* factors, const double* src, int64_t src_stride, bool dev,
                      bool vectors, const char* wrong_kind, DevBuf<Rec>& d_recs, Fill&& fill) {
  const Plan& p = e->model.plan->p;
  std::vector<uint8_t> seen((size_t)p.nf, 0);
  std::vector<Rec> recs((size_t)n);
  int64_t longest = 0, total = 0;
  int32_t longest_f = -1;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t f = factors[i];
    if (f < 0 || f >= p.nf) throw std::runtime_error(who + ": factor index " + std::to_string(f) + " (entry " + std::to_string(i) + ") is out of range");
    if ((p.f_kind[f] == LPMP_F_VECTOR) != vectors) throw std::runtime_error(who + ": factor " + std::to_string(f) + wrong_kind);
    if (seen[(size_t)f]) throw std::runtime_error(who + ": factor " + std::to_string(f) + " is listed twice (the result would depend on the order of two waves)");
    seen[(size_t)f] = 1;
    // (a host source is packed row after row: stride 1, row = offset)
    const Rec r = fill(i, f, dev ? i : total);
    if (r.len > longest) { longest = r.len; longest_f = f; }
    recs[(size_t)i] = r;
    total += r.len;
  }
  if (n > 0 && src_stride < longest)
    throw std::runtime_error(who + ": src_stride " + std::to_string(src_stride) + " is smaller than the " + std::to_string(longest) + " entries of factor " + std::to_string(longest_f));
  settle(e);
  check_chain(e);
  if (n == 0) return {nullptr, 0};
  d_recs.grow((size_t)n);
  h2d(d_recs, recs.data(), (size_t)n * sizeof(Rec), e->stream);
  if (dev) return {src, src_stride};
  std::vector<double> rows((size_t)total);
  for (int64_t i = 0; i < n; ++i) std::copy(src + i * src_stride, src + i * src_stride + recs[(size_t)i].len, rows.begin() + recs[(size_t)i].src_row);
  e->model.d_setsrc.grow((size_t)total);
  h2d(e->model.d_setsrc, rows.data(), (size_t)total * sizeof(double), e->stream);
  return {e->model.d_setsrc.get(), 1};
}
}  // namespace

// (the lpmp_* functions below have C linkage from their declarations in include/lpmp_engine.h and engine_internal.h)
// ---- plan -----------------------------------------------------------------------------------------
int lpmp_plan_create(const lpmp_model* m, lpmp_plan** out) {
  return guarded([&] {
    if (!m || !out) throw std::runtime_error("null argument");
    auto p = std::make_unique<lpmp_plan>();
    p->p.build(*m);
    *out = p.release();
  });
}
void lpmp_plan_destroy(lpmp_plan* p) { delete p; }
int64_t lpmp_plan_n_factors(const lpmp_plan* p) { return p ? p->p.nf : 0; }
int64_t lpmp_plan_n_updated(const lpmp_plan* p, int d) { return p && (d == 0 || d == 1) ? (int64_t)p->p.upd[d].size() : 0; }
int lpmp_plan_get_order(const lpmp_plan* p, int d, int32_t* out) {
  return guarded([&] {
    if (!p || !out || d < 0 || d > 1) throw std::runtime_error("bad argument");
    std::memcpy(out, p->p.order[d].data(), p->p.order[d].size() * sizeof(int32_t));
  });
}
int lpmp_plan_get_update_order(const lpmp_plan* p, int d, int32_t* out) {
  return guarded([&] {
    if (!p || !out || d < 0 || d > 1) throw std::runtime_error("bad argument");
    std::memcpy(out, p->p.upd[d].data(), p->p.upd[d].size() * sizeof(int32_t));
  });
}
int64_t lpmp_plan_omega_nnz(lpmp_plan* p, int d) {
  int64_t s = 0;
  if (p && (d == 0 || d == 1)) for (int32_t f : p->p.upd[d]) s += p->p.row_sends(f);
  return s;
}
int64_t lpmp_plan_mask_nnz(lpmp_plan* p, int d) {
  int64_t s = 0;
  if (p && (d == 0 || d == 1)) for (int32_t f : p->p.upd[d]) s += p->p.row_receives(f);
  return s;
}
int lpmp_plan_get_omega(lpmp_plan* p, int d, int mode, int64_t* off, double* data) {
  return guarded([&] {
    if (!p || !off || d < 0 || d > 1) throw std::runtime_error("bad argument");
    p->p.ensure_weights(mode);
    const auto& c = p->p.omega[d][mode];
    std::memcpy(off, c.off.data(), c.off.size() * sizeof(int64_t));
    if (!c.data.empty()) std::memcpy(data, c.data.data(), c.data.size() * sizeof(double));
  });
}
int lpmp_plan_get_mask(lpmp_plan* p, int d, int mode, int64_t* off, uint8_t* data) {
  return guarded([&] {
    if (!p || !off || d < 0 || d > 1) throw std::runtime_error("bad argument");
    p->p.ensure_weights(mode);
    const auto& c = p->p.mask[d][mode];
    std::memcpy(off, c.off.data(), c.off.size() * sizeof(int64_t));
    if (!c.data.empty()) std::memcpy(data, c.data.data(), c.data.size());
  });
}
int lpmp_plan_get_msg_lists(const lpmp_plan* p, int64_t* off, int64_t* entries) {
  return guarded([&] {
    if (!p || !off || !entries) throw std::runtime_error("bad argument");
    std::memcpy(off, p->p.fm_off.data(), p->p.fm_off.size() * sizeof(int64_t));
    for (size_t i = 0; i < p->p.fm.size(); ++i) entries[i] = (int64_t)p->p.fm[i].msg * 2 + p->p.fm[i].role;
  });
}
int lpmp_plan_anisotropic_weights(const lpmp_plan* p, int64_t n, const int32_t* factors, int64_t* n_rows, int64_t* om_nnz,
                                  int64_t* mk_nnz, int64_t* om_off, double* om, int64_t* mk_off, uint8_t* mk) {
  return guarded([&] {
    if (!p || !factors || n < 0) throw std::runtime_error("bad argument");
    Csr<double> a; Csr<uint8_t> b;
    p->p.anisotropic_weights(factors, n, a, b);
    if (n_rows) *n_rows = a.rows();
    if (om_nnz) *om_nnz = (int64_t)a.data.size();
    if (mk_nnz) *mk_nnz = (int64_t)b.data.size();
    if (om_off && om && mk_off && mk) {
      std::memcpy(om_off, a.off.data(), a.off.size() * sizeof(int64_t));
      std::memcpy(mk_off, b.off.data(), b.off.size() * sizeof(int64_t));
      if (!a.data.empty()) std::memcpy(om, a.data.data(), a.data.size() * sizeof(double));
      if (!b.data.empty()) std::memcpy(mk, b.data.data(), b.data.size());
    }
  });
}
int lpmp_plan_schedule_info(lpmp_plan* p, int d, int mode, int64_t* n_levels, int64_t* n_launches, int64_t* n_recv,
                            int64_t* n_send, int64_t* alg_bytes) {
  return guarded([&] {
    if (!p || d < 0 || d > 1 || mode < 0 || mode >= LPMP_REPAM_COUNT) throw std::runtime_error("bad argument");
    plan_schedule(p, d, mode);
    const Schedule& s = p->sched_cache[d][mode];
    if (n_levels) *n_levels = s.n_levels;
    if (n_launches) *n_launches = (int64_t)s.launches.size();
    if (n_recv) *n_recv = s.n_recv;
    if (n_send) *n_send = s.n_send;
    if (alg_bytes) *alg_bytes = s.alg_bytes;
  });
}

int lpmp_plan_schedule_classes(lpmp_plan* p, int d, int mode, int64_t* factors) {
  static_assert(LPMP_KCLASS_COUNT == KC_COUNT, "public class count");
  return guarded([&] {
    if (!p || !factors || d < 0 || d > 1 || mode < 0 || mode >= LPMP_REPAM_COUNT) throw std::runtime_error("bad argument");
    plan_schedule(p, d, mode);
    for (int c = 0; c < KC_COUNT; ++c) factors[c] = 0;
    for (const auto& lr : p->sched_cache[d][mode].launches) factors[lr.kclass] += lr.end - lr.begin;
  });
}

int lpmp_plan_n_shared_tables(const lpmp_plan* p) { return p ? p->p.n_shared : 0; }
int lpmp_plan_get_diff_band(const lpmp_plan* p, int table, int32_t* lo, int32_t* hi, int* banded) {
  return guarded([&] {
    if (!p || table < 0 || table >= p->p.n_shared) throw std::runtime_error("bad argument");
    const bool diff = p->p.sh_banded[(size_t)table] >= 0;
    if (lo) *lo = diff ? p->p.sh_lo[(size_t)table] : 0;
    if (hi) *hi = diff ? p->p.sh_hi[(size_t)table] : -1;
    if (banded) *banded = p->p.sh_banded[(size_t)table];
  });
}
int lpmp_plan_get_diff_shift_band(const lpmp_plan* p, int table, int32_t* lo, int32_t* hi, int* referenced) {
  return guarded([&] {
    if (!p || table < 0 || table >= p->p.n_shared) throw std::runtime_error("bad argument");
    const bool ref = p->p.sh_shift_ref[(size_t)table] != 0;
    if (lo) *lo = ref ? p->p.sh_lo[(size_t)table] : 0;
    if (hi) *hi = ref ? p->p.sh_hi[(size_t)table] : -1;
    if (referenced) *referenced = ref ? 1 : 0;
  });
}
int lpmp_plan_set_shared_pool(lpmp_plan* p, const double* sh_data) {
  return guarded([&] {
    if (!p || !sh_data) throw std::runtime_error("lpmp_plan_set_shared_pool: null argument");
    p->set_shared_pool(sh_data);
  });
}
int lpmp_plan_diff_band_info(lpmp_plan* p, int d, int mode, int64_t* diff_launches, int64_t* band_launches, int64_t* diff_receives,
                             int64_t* band_receives) {
  return guarded([&] {
    if (!p || d < 0 || d > 1 || mode < 0 || mode >= LPMP_REPAM_COUNT) throw std::runtime_error("bad argument");
    plan_schedule(p, d, mode);
    int64_t v[4] = {0, 0, 0, 0};
    for (const auto& lr : p->sched_cache[d][mode].launches)
      if (lr.kclass == KC_DIFF) { ++v[0]; v[2] += lr.n_recv; if (lr.diff_band) { ++v[1]; v[3] += lr.n_recv; } }
    if (diff_launches) *diff_launches = v[0];
    if (band_launches) *band_launches = v[1];
    if (diff_receives) *diff_receives = v[2];
    if (band_receives) *band_receives = v[3];
  });
}

int lpmp_plan_diff_shift_band_info(lpmp_plan* p, int d, int mode, int64_t* shift_launches, int64_t* shift_band_launches, int64_t* shift_receives,
                                   int64_t* shift_band_receives) {
  return guarded([&] {
    if (!p || d < 0 || d > 1 || mode < 0 || mode >= LPMP_REPAM_COUNT) throw std::runtime_error("bad argument");
    plan_schedule(p, d, mode);
    int64_t v[4] = {0, 0, 0, 0};
    for (const auto& lr : p->sched_cache[d][mode].launches)
      if (lr.kclass == KC_DIFF && lr.diff_shift) { ++v[0]; v[2] += lr.n_recv; if (lr.diff_shift_band) { ++v[1]; v[3] += lr.n_recv; } }
    if (shift_launches) *shift_launches = v[0];
    if (shift_band_launches) *shift_band_launches = v[1];
    if (shift_receives) *shift_receives = v[2];
    if (shift_band_receives) *shift_band_receives = v[3];
  });
}

int lpmp_plan_custom_schedule_info(lpmp_plan* p, int64_t n, const int32_t* factors, const int64_t* om_off, const double* om,
                                   const int64_t* mk_off, const uint8_t* mk, int fuse, int64_t* n_levels, int64_t* n_launches,
                                   int64_t* n_recv, int64_t* n_send, int64_t* alg_bytes) {
  return guarded([&] {
    if (!p || n < 0 || (n > 0 && (!factors || !om_off || !mk_off))) throw std::runtime_error("bad argument");
    check_rows(n, om_off, om, mk_off, mk);
    Schedule s;
    static const double dz = 0; static const uint8_t uz = 0;
    static const int64_t zero_off[1] = {0};
    p->p.make_schedule(std::vector<Plan::Segment>{Plan::Segment{factors, n, n > 0 ? om_off : zero_off, om ? om : &dz,
                                                                n > 0 ? mk_off : zero_off, mk ? mk : &uz}}, fuse != 0, s);
    if (n_levels) *n_levels = s.n_levels;
    if (n_launches) *n_launches = (int64_t)s.launches.size();
    if (n_recv) *n_recv = s.n_recv;
    if (n_send) *n_send = s.n_send;
    if (alg_bytes) *alg_bytes = s.alg_bytes;
  });
}

int lpmp_plan_get_update_levels(lpmp_plan* p, int d, int mode, int32_t* out) {
  return guarded([&] {
    if (!p || !out || d < 0 || d > 1 || mode < 0 || mode >= LPMP_REPAM_COUNT) throw std::runtime_error("bad argument");
    if (!p->have_sched[d][mode]) {
      // the sweep has not been planned (a multi-GPU host asking for the GLOBAL level structure never runs it): the levels alone
      p->p.ensure_weights(mode);
      const auto& om = p->p.omega[d][mode];
      const auto& mk = p->p.mask[d][mode];
      std::vector<int32_t> lv;
      Schedule scratch;
      p->p.make_schedule(std::vector<Plan::Segment>{{p->p.upd[d].data(), (int64_t)p->p.upd[d].size(), om.off.data(), om.data.data(), mk.off.data(), mk.data.data()}},
                         false, scratch, false, &lv);
      std::copy(lv.begin(), lv.end(), out);
      return;
    }
    const Schedule& s = p->sched_cache[d][mode];
    std::vector<int32_t> level_of(p->p.nf, 0);
    for (const auto& lr : s.launches) for (int64_t i = lr.begin; i < lr.end; ++i) level_of[s.recs[i].factor] = lr.level;
    const auto& upd = p->p.upd[d];
    for (size_t i = 0; i < upd.size(); ++i) out[i] = level_of[upd[i]];
  });
}

// the decode structure of a direction, or the planner's refusal
static const DecodePlan& decode_plan_or_refuse(lpmp_plan* p, int d) {
  const DecodePlan& dp = p->decode(d);
  if (!dp.why.empty()) throw UnsupportedError(dp.why);
  return dp;
}
int lpmp_plan_decode_info(lpmp_plan* p, int d, int64_t* n_unaries, int64_t* n_levels, int64_t* n_links) {
  return guarded([&] {
    if (!p || d < 0 || d > 1) throw std::runtime_error("bad argument");
    const DecodePlan& dp = decode_plan_or_refuse(p, d);
    if (n_unaries) *n_unaries = (int64_t)dp.unaries.size();
    if (n_levels) *n_levels = dp.n_levels;
    if (n_links) *n_links = (int64_t)dp.edges.size();
  });
}
int lpmp_plan_get_decode_levels(lpmp_plan* p, int d, int32_t* factor_out, int32_t* level_out) {
  return guarded([&] {
    if (!p || d < 0 || d > 1 || !factor_out || !level_out) throw std::runtime_error("bad argument");
    const DecodePlan& dp = decode_plan_or_refuse(p, d);
    std::copy(dp.unaries.begin(), dp.unaries.end(), factor_out);
    std::copy(dp.level.begin(), dp.level.end(), level_out);
  });
}

int lpmp_plan_suggest_order(lpmp_plan* p, uint64_t seed, int32_t* rank_of_factor, int32_t* n_colours) {
  return guarded([&] {
    if (!p || (!rank_of_factor && p->p.nf > 0)) throw std::runtime_error("null argument");
    const int32_t k = suggest_order(p->p, seed, rank_of_factor);
    if (n_colours) *n_colours = k;
  });
}
int lpmp_plan_pass_schedule_info(lpmp_plan* p, int mode, int64_t* n_levels, int64_t* n_launches, int64_t* n_recv,
                                 int64_t* n_send, int64_t* alg_bytes) {
  return guarded([&] {
    if (!p || mode < 0 || mode >= LPMP_REPAM_COUNT) throw std::runtime_error("bad argument");
    plan_pass_schedule(p, mode);
    const Schedule& s = p->pass_cache[mode];
    if (n_levels) *n_levels = s.n_levels;
    if (n_launches) *n_launches = (int64_t)s.launches.size();
    if (n_recv) *n_recv = s.n_recv;
    if (n_send) *n_send = s.n_send;
    if (alg_bytes) *alg_bytes = s.alg_bytes;
  });
}

int lpmp_plan_chain_info(lpmp_plan* p, int d, int mode, int64_t* n_chains, int64_t* n_tickets, int64_t* n_dependencies, int64_t* n_plain_launches) {
  return guarded([&] {
    if (!p || mode < 0 || mode >= LPMP_REPAM_COUNT || d < -1 || d > 1) throw std::runtime_error("bad argument");
    const Schedule* s;
    if (d < 0) { plan_pass_schedule(p, mode); s = &p->pass_cache[mode]; } else { plan_schedule(p, d, mode); s = &p->sched_cache[d][mode]; }
    int64_t t = 0, e = 0;
    for (const auto& c : s->chains) { t += (int64_t)c.tk_launch.size(); e += (int64_t)c.dep.size(); }
    if (n_chains) *n_chains = (int64_t)s->chains.size();
    if (n_tickets) *n_tickets = t;
    if (n_dependencies) *n_dependencies = e;
    if (n_plain_launches) *n_plain_launches = (int64_t)s->plain_launches.size();
  });
}

int lpmp_plan_mailbox_info(lpmp_plan* p, int d, int mode, int64_t* n_rows, int64_t* n_receives) {
  return guarded([&] {
    if (!p || mode < 0 || mode >= LPMP_REPAM_COUNT || d < -1 || d > 1) throw std::runtime_error("bad argument");
    const Schedule* s;
    if (d < 0) { plan_pass_schedule(p, mode); s = &p->pass_cache[mode]; } else { plan_schedule(p, d, mode); s = &p->sched_cache[d][mode]; }
    int64_t r = 0, v = 0;
    for (const auto& c : s->chains) { r += c.mailbox_rows; v += c.mailbox_receives; }
    if (n_rows) *n_rows = r;
    if (n_receives) *n_receives = v;
  });
}

// which body every launch of a level loop takes (kernels.hip, level_loop_kernel): read from the flags chain_plan.cpp set, nothing planned
// beyond what lpmp_plan_chain_info plans
int lpmp_plan_level_loop_info(lpmp_plan* p, int d, int mode, int64_t* n_launches, int64_t* n_lane_launches, int64_t* n_label_ops,
                              int64_t* n_label_paired, int64_t* n_label_staged, int64_t* n_label_paired_staged) {
  return guarded([&] {
    if (!p || mode < 0 || mode >= LPMP_REPAM_COUNT || d < -1 || d > 1) throw std::runtime_error("bad argument");
    const Schedule* s;
    if (d < 0) { plan_pass_schedule(p, mode); s = &p->pass_cache[mode]; } else { plan_schedule(p, d, mode); s = &p->sched_cache[d][mode]; }
    int64_t n = 0, lane = 0, ops = 0, paired = 0, staged = 0, paired_staged = 0;
    for (const auto& c : s->chains) {
      if (!c.level_loop) continue;
      n += (int64_t)c.launches.size();
      if (c.kclass != KC_SMALL) continue;
      lane += (int64_t)c.launches.size();
      for (const auto& cl : c.launches) {
        if (!(cl.flags & CHAIN_LAUNCH_LABEL_OPS)) continue;
        const bool pr = (cl.flags & CHAIN_LAUNCH_LABEL_PAIRED) != 0, st = cl.count <= LL_STAGE_RECS;
        ++ops; paired += pr; staged += st; paired_staged += pr && st;
      }
    }
    if (n_launches) *n_launches = n;
    if (n_lane_launches) *n_lane_launches = lane;
    if (n_label_ops) *n_label_ops = ops;
    if (n_label_paired) *n_label_paired = paired;
    if (n_label_staged) *n_label_staged = staged;
    if (n_label_paired_staged) *n_label_paired_staged = paired_staged;
  });
}

int lpmp_plan_get_partitions(lpmp_plan* p, int64_t* n_partitions, int64_t* off, int32_t* factors) {
  return guarded([&] {
    if (!p || !n_partitions) throw std::runtime_error("bad argument");
    p->p.ensure_partition();
    const auto& pt = p->p.part;
    *n_partitions = (int64_t)pt.off.size() - 1;
    if (off && factors) {
      std::memcpy(off, pt.off.data(), pt.off.size() * sizeof(int64_t));
      if (!pt.f.empty()) std::memcpy(factors, pt.f.data(), pt.f.size() * sizeof(int32_t));
    }
  });
}

int lpmp_plan_pass_rotates(lpmp_plan* p, int mode) {
  int r = 0;
  const int rc = guarded([&] {
    if (!p || mode < 0 || mode >= LPMP_REPAM_COUNT) throw std::runtime_error("bad argument");
    if (!p->have_bf[mode]) { plan_pass_schedule(p, mode); if (p->pass_cache[mode].recs.empty() && !p->pass_cache[mode].launches.empty()) throw StateError("pass schedule already handed to the device"); plan_rotation(p, mode); }
    r = p->rotation_ok[mode] ? 1 : 0;
  });
  return rc == LPMP_OK ? r : rc;
}

// may the joined passes of a mode take the peer-minima form, as far as the STRUCTURE decides (RotationInfo::peer_minima; the engine
// adds: f64 tables, packed layout, LPMP_NO_PEER_MINIMA unset)?  1 / 0, or an error code; why (n bytes, may be null): "" or the obstacle
int lpmp_plan_peer_minima(lpmp_plan* p, int mode, char* why, int n) {
  int r = 0;
  const int rc = guarded([&] {
    if (!p || mode < 0 || mode >= LPMP_REPAM_COUNT) throw std::runtime_error("bad argument");
    std::string reason;
    if (p->rot[mode].valid) { r = p->rot[mode].peer_minima ? 1 : 0; reason = p->rot[mode].peer_minima_why; }
    else {
      if (!p->have_bf[mode]) { plan_pass_schedule(p, mode); if (p->pass_cache[mode].recs.empty() && !p->pass_cache[mode].launches.empty()) throw StateError("pass schedule already handed to the device"); plan_rotation(p, mode); }
      if (!p->rotation_ok[mode]) reason = "the passes of this mode do not join";
      else if (p->pass_cache[mode].recs.empty() || p->bf_cache[mode].recs.empty()) throw StateError("pass schedule already handed to the device");
      else {
        const RotationInfo ri = plan_rotation_chain(p->pass_cache[mode], p->bf_cache[mode], p->p.nf);
        r = ri.valid && ri.peer_minima ? 1 : 0;
        reason = ri.valid ? ri.peer_minima_why : "the pass does not have the H, W, K, T shape of one packed class";
      }
    }
    if (why && n > 0) { std::snprintf(why, (size_t)n, "%s", reason.c_str()); }
  });
  return rc == LPMP_OK ? r : rc;
}

// ---- engine ---------------------------------------------------------------------------------------
int lpmp_create(int device, lpmp_engine** out) {
  return guarded([&] {
    if (!out) throw std::runtime_error("null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw DeviceError("no HIP device available: the engine has no CPU path");
    if (device < 0 || device >= n) throw DeviceError("device ordinal out of range");
    HIP_CHECK(hipSetDevice(device));
    auto e = std::make_unique<lpmp_engine>();
    e->device = device;
    e->stream = stream_pool().take(device);
    e->own_stream = true;
    const char* ng = std::getenv("LPMP_NO_GRAPH");
    e->use_graph = !(ng && ng[0] == '1');
    const char* nf = std::getenv("LPMP_NO_FUSE");
    e->use_fused = !(nf && nf[0] == '1');
    const char* nr = std::getenv("LPMP_NO_ROTATION");
    e->use_rotation = !(nr && nr[0] == '1');
    const char* nt = std::getenv("LPMP_NO_LB_TRACKING");
    e->use_lb_tracking = !(nt && nt[0] == '1');
    const char* nc = std::getenv("LPMP_NO_CHAIN");
    e->use_chain = !(nc && nc[0] == '1');
    const char* nb = std::getenv("LPMP_NO_BLOCKED_PASSES");
    e->use_blocked_passes = !(nb && nb[0] == '1');
    const char* np = std::getenv("LPMP_NO_PEER_MINIMA");
    e->use_peer_minima = !(np && np[0] == '1');
    if (const char* v = std::getenv("LPMP_PQ_LDS")) e->pq_lds = v[0] == '0' ? 0 : 1;
    if (const char* v = std::getenv("LPMP_PQ_HOLD")) e->pq_hold = v[0] == '2' ? 2 : 3;
    if (const char* v = std::getenv("LPMP_PQ_SCATTER")) e->pq_scatter = v[0] != '0';
    if (const char* v = std::getenv("LPMP_PQ_WIDE")) e->pq_wide = v[0] != '0';
    if (const char* v = std::getenv("LPMP_PQ_AHEAD")) e->pq_ahead = v[0] == '0' ? 0 : v[0] == '2' ? 2 : 1;
    if (const char* v = std::getenv("LPMP_PQ_DESC_INLINE")) e->pq_desc_inline = std::min(std::max(0, std::atoi(v)), TICKET_DESC_INLINE);
    if (const char* v = std::getenv("LPMP_CHAIN_MAX_WGS")) e->chain_max_wgs = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("LPMP_PQ_TILES")) e->pq_tiles = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("LPMP_PQ_SUB")) e->pq_sub = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("LPMP_PQ_SUBLAG")) e->pq_sublag = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("LPMP_PQ_SUBGAP")) e->pq_subgap = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("LPMP_PQ_MIN_PASSES")) e->pq_min_passes = std::max(1, std::atoi(v));
    if (const char* v = std::getenv("LPMP_ROT_BANDS")) e->rot_opts.bands = std::atoi(v);
    if (const char* v = std::getenv("LPMP_ROT_LAG")) { e->rot_opts.lag = std::max(1, std::atoi(v)); e->rot_opts.lag_set = true; }
    if (const char* v = std::getenv("LPMP_ROT_DEPTH")) { e->rot_opts.depth = std::max(1, std::atoi(v)); e->rot_opts.depth_set = true; }
    if (const char* v = std::getenv("LPMP_ROT_TILES")) { e->rot_tiles = std::max(0, std::atoi(v)); e->rot_tiles_set = true; }
    if (const char* v = std::getenv("LPMP_CHAIN_CACHE_MB")) e->rot_cache_limit = (size_t)std::max(1, std::atoi(v)) << 20;
    if (const char* v = std::getenv("LPMP_ROWS_LAYOUT")) e->want_rows = std::atoi(v) != 0;                             // as lpmp_set_rows_layout
    if (const char* v = std::getenv("LPMP_SPECULATION")) e->spec.max_depth = std::min(32, std::max(0, std::atoi(v)));   // as lpmp_set_speculation
    *out = e.release();
  });
}

void lpmp_destroy(lpmp_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  // a BORROWED dual buffer (LPMP_MEM_DEVICE) outlives the engine: an open batch of passes that ran ahead of the caller must
  // not stay in it
  if (e->model.plan && !e->model.own_dual() && e->model.batch.n > 0) { try { settle(e); } catch (const std::exception& ex) { std::fprintf(stderr, "lpmp_destroy: could not roll back passes that ran ahead: %s\n", ex.what()); } }
  (void)hipStreamSynchronize(e->stream);
  for (auto& p : e->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  for (auto ev : e->event_pool) (void)hipEventDestroy(ev);
  e->release_model();
  e->d_chain_abort.reset();
  if (e->own_stream && e->stream) stream_pool().give(e->device, e->stream);
  if (e->capture_stream) { (void)hipStreamSynchronize(e->capture_stream); stream_pool().give(e->device, e->capture_stream); }
  if (!guarded_ok(e->pinned, PINNED_WORDS_BYTES)) {   // a damaged block is reported and never reused
    std::fprintf(stderr, "lpmp_destroy: guard region of the engine's pinned words was overwritten\n");
    g_error = "guard region of the engine's pinned words was overwritten";
  } else pinned_pool().give(e->pinned);
  delete e;
}

int lpmp_set_stream(lpmp_engine* e, void* s) {
  return guarded([&] {
    if (!e) throw std::runtime_error("null engine");
    settle(e);
    HIP_CHECK(hipStreamSynchronize(e->stream));
    for (int d = 0; d < 2; ++d) for (int m = 0; m < LPMP_REPAM_COUNT; ++m)
      e->model.sched[d][m].graph.reset();
    for (int m = 0; m < LPMP_REPAM_COUNT; ++m)
      e->model.sched_pass[m].graph.reset();
    if (e->own_stream && e->stream) stream_pool().give(e->device, e->stream);
    e->stream = (hipStream_t)s; e->own_stream = false;
  });
}

// the one sentence that refuses an entry a float table cannot hold (the upload and lpmp_upload_costs: a table; lpmp_set_constants: a row)
static std::string f32_refusal(const char* who, bool strict, const char* what, int factor, const char* tail) {
  return std::string(who) + "table precision " + (strict ? "f32" : "f32_round") + ": the " + what + " of factor " + std::to_string(factor) +
         (strict ? " holds an entry that is not exactly a float (or a finite one beyond float's range or below FLT_MIN)"
                 : " holds a finite entry beyond float's range or a nonzero one below FLT_MIN") + tail;
}

// Table precision f32 (lpmp_set_table_precision): every DENSE table of the packed constants becomes floats in m.d_tab32, each
// table 16-byte aligned, and p.dev_coff[f] of a DENSE factor its place there (8-byte units relative to m.d_const).
//   on_device: `consts` is the caller's device buffer — it stays m.d_const, the tables are narrowed out of it, and afterwards
//     the engine reads only the cells of the other factors from it.
//   otherwise `consts` is host memory: the tables pass through a staging buffer of at most 256 MiB, chunk by chunk, and are never
//     resident as doubles as a whole; the cells of the other factors (Potts, SHARED and DIFF scalars) are gathered into a compact
//     buffer of doubles that becomes m.d_const (m.tab_compact), and dev_coff of those factors points into it.
// Throws UnsupportedError naming the lowest DENSE factor that holds an entry the mode refuses (kernels.hip, narrow_tables_kernel).
// The mode is m.tab_prec.  fresh (the upload): the buffers are allocated and dev_coff is laid out.  Not fresh (lpmp_upload_costs):
// the same narrowing into the buffers and offsets of the upload — `consts` is m.d_const itself (a borrowed buffer, already holding
// the new constants) or, for a model whose compact buffer came from host memory, host or device memory of the caller's.
static void narrow_tables(ModelState& m, hipStream_t stream, const double* consts, bool on_device, bool fresh = true) {
  Plan& p = m.plan->p;
  const int strict = m.tab_prec == LPMP_TABLES_F32 ? 1 : 0;
  const bool compact = m.tab_compact;
  std::vector<NarrowRec> recs;
  std::vector<double> small;
  struct Run { int64_t src, dst, n; };
  std::vector<Run> runs;                           // compact cells out of a device buffer: runs of consecutive non-DENSE factors
  if (fresh) p.dev_coff.assign(p.f_coff.begin(), p.f_coff.end());
  int64_t at = 0, small_at = 0;                    // floats; doubles of the compact buffer
  for (int64_t f = 0; f < p.nf; ++f) {
    const int64_t n = p.f_coff[f + 1] - p.f_coff[f];
    if (p.f_kind[f] == LPMP_F_PAIRWISE_DENSE) {
      recs.push_back({p.f_coff[f], at, n, (int32_t)f, 0});
      at += (n + 3) / 4 * 4;
    } else if (compact) {
      if (fresh) p.dev_coff[f] = small_at;
      if (!on_device) small.insert(small.end(), consts + p.f_coff[f], consts + p.f_coff[f + 1]);
      else if (n > 0) { if (!runs.empty() && runs.back().src + runs.back().n == p.f_coff[f]) runs.back().n += n; else runs.push_back({p.f_coff[f], small_at, n}); }
      small_at += n;
    }
  }
  if (compact) {
    if (fresh) { m.const_buf.alloc(std::max<size_t>(2, (size_t)small_at)); m.d_const = m.const_buf; }
    else if ((size_t)small_at > m.const_buf.capacity()) throw std::runtime_error("table precision: the compact constants do not fit their buffer");
    if (!small.empty()) h2d(m.d_const, small.data(), small.size() * sizeof(double), stream);
    for (const Run& r : runs) HIP_CHECK(hipMemcpyAsync(m.const_buf + r.dst, consts + r.src, (size_t)r.n * sizeof(double), hipMemcpyDeviceToDevice, stream));
  }
  if (recs.empty()) return;
  if (!fresh) { if ((size_t)at > m.d_tab32.capacity()) throw std::runtime_error("table precision: the tables do not fit their buffer"); }
  else {
  m.d_tab32.alloc((size_t)at);
  if ((((uintptr_t)m.d_tab32.get() - (uintptr_t)m.d_const) % 16) != 0) throw std::runtime_error("table precision: buffers are not aligned to each other");
  const int64_t shift = (int64_t)(((intptr_t)m.d_tab32.get() - (intptr_t)m.d_const) / 8);
  for (const NarrowRec& r : recs) p.dev_coff[r.factor] = shift + r.dst_off / 2;
  }
  DevBuf<int> d_bad; d_bad.alloc(1);
  const int none = INT32_MAX;
  h2d(d_bad, &none, sizeof(int), stream);
  DevBuf<NarrowRec> d_recs;
  if (on_device) {
    d_recs.alloc(recs.size());
    h2d(d_recs, recs.data(), recs.size() * sizeof(NarrowRec), stream);
    launch_narrow_tables(d_recs, (int64_t)recs.size(), consts, m.d_tab32, strict, d_bad, stream);
    HIP_CHECK(hipGetLastError());
  } else {
    // chunks of whole tables, at most STAGE doubles of the packed array each (a table has at most BIG_MAX_LABELS^2 entries: 2 MiB)
    const int64_t STAGE = ((int64_t)256 << 20) / (int64_t)sizeof(double);
    int64_t span = 0, cnt = 0;
    for (size_t a = 0; a < recs.size();) {        // the largest chunk: sizes the two device buffers once
      size_t b = a; const int64_t c0 = recs[a].src_off;
      while (b < recs.size() && recs[b].src_off + recs[b].n - c0 <= STAGE) ++b;
      if (b == a) throw std::runtime_error("table precision: a table larger than the staging buffer");
      span = std::max(span, recs[b - 1].src_off + recs[b - 1].n - c0); cnt = std::max(cnt, (int64_t)(b - a));
      a = b;
    }
    DevBuf<double> stage; stage.alloc((size_t)span);
    d_recs.alloc((size_t)cnt);
    std::vector<NarrowRec> part;
    for (size_t a = 0; a < recs.size();) {
      size_t b = a; const int64_t c0 = recs[a].src_off;
      while (b < recs.size() && recs[b].src_off + recs[b].n - c0 <= STAGE) ++b;
      part.assign(recs.begin() + (std::ptrdiff_t)a, recs.begin() + (std::ptrdiff_t)b);
      for (NarrowRec& r : part) r.src_off -= c0;
      h2d(stage, consts + c0, (size_t)(recs[b - 1].src_off + recs[b - 1].n - c0) * sizeof(double), stream);
      h2d(d_recs, part.data(), part.size() * sizeof(NarrowRec), stream);
      launch_narrow_tables(d_recs, (int64_t)part.size(), stage, m.d_tab32, strict, d_bad, stream);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipStreamSynchronize(stream));   // `part` and the staging buffer are reused by the next chunk
      a = b;
    }
  }
  int bad = none;
  d2h(&bad, d_bad, sizeof(int), stream);
  HIP_CHECK(hipStreamSynchronize(stream));
  if (bad != none) throw UnsupportedError(f32_refusal("", strict != 0, "table", bad, ""));
}

// The engine-private copies of the constants that are COSTS, not structure: lpmp_upload_model derives them once, lpmp_upload_costs
// again, with these functions (and narrow_tables above).
// SHARED / DIFF factors: the cells {const offset of the factor's scale, table offset} go to the device as the upload laid them out
// and shared_cells_kernel replaces every first word by the scale it finds in the constants; the pool behind the cells is not touched.
// A DIFF_SHIFT factor has a second cell right behind the first, {const offset of its shift, n = the length of D}: the same kernel
// gathers the shift as it gathers a scale, and the factor's four words on the device are {scale, offset of D, shift (the double
// of the constants: the kernels convert it, kernels.hip diff_shift_int), n}
static void gather_shared_cells(ModelState& m, hipStream_t stream) {
  if (m.sh_cells.empty()) return;
  h2d(m.d_shared, m.sh_cells.data(), m.sh_cells.size() * sizeof(int64_t), stream);
  launch_shared_cells(m.d_shared, (int64_t)m.sh_cells.size() / 2, m.d_const, stream);
  HIP_CHECK(hipGetLastError());
}
// ... the pool block of d_shared, behind the n_sf cells (two words each): every entry t of the plan's pool with one 8-byte band word
// {int32 lo, int32 hi} in front of it — sweep_diff_band_kernel and sweep_diff_shift_band_kernel learn the band of a DIFF / DIFF_SHIFT
// vector from the word before the offset in the factor's cell (entries neither kind references: an empty band, never read; the plan
// keeps sh_lo / sh_hi for both kinds, so new pool values rewrite the word of a shift-only entry too).  Entry t starts at shared_pool_at(p, t).
static int64_t shared_pool_at(const Plan& p, int32_t t) { return p.sh_off[(size_t)t] + t + 1; }
static void write_shared_pool(ModelState& m, hipStream_t stream, int64_t n_sf) {
  const Plan& p = m.plan->p;
  const int64_t n_pool = p.sh_off[(size_t)p.n_shared] + p.n_shared;
  if ((size_t)(2 * n_sf + n_pool) > m.d_shared.capacity()) throw std::runtime_error("shared tables: the pool does not fit its buffer");
  std::vector<double> pool((size_t)n_pool);
  for (int32_t t = 0; t < p.n_shared; ++t) {
    const int32_t word[2] = {p.sh_lo[(size_t)t], p.sh_hi[(size_t)t]};
    static_assert(sizeof word == sizeof(double), "band word");
    std::memcpy(&pool[(size_t)(shared_pool_at(p, t) - 1)], word, sizeof word);
    std::copy(p.sh_data.begin() + p.sh_off[(size_t)t], p.sh_data.begin() + p.sh_off[(size_t)t + 1], pool.begin() + shared_pool_at(p, t));
  }
  h2d(m.d_shared + 2 * n_sf, pool.data(), (size_t)n_pool * sizeof(double), stream);
}
// rows layout: every row [table | m1 | m2] from the packed constants and the packed duals
static void build_rows(ModelState& m, hipStream_t stream) {
  launch_rows_copy(m.d_rowrecs, m.n_rowrecs, m.d_const, m.d_dual, m.d_rows, 0, stream);
  HIP_CHECK(hipGetLastError());
}

// what keeps a model from running under a send rule (also checked at upload: the rule may be set first,
// as the reference parses --reparametrizationType in LP::Begin)
static void check_rtype(const ModelState& m, int rtype) {
  if (!m.plan) return;
  const Plan& p = m.plan->p;
  if (rtype == LPMP_RTYPE_RESIDUAL && p.any_batch)
    throw UnsupportedError("residual sends with batch-capable message ops are not built (send_messages_residual's batch branch, factors_messages.hxx:2980-2991)");
  if (rtype == LPMP_RTYPE_ADAPTIVE) { const std::string why = p.adaptive_obstacle(); if (!why.empty()) throw UnsupportedError(why); }
}

// ---- the layout steps of lpmp_upload_model: each fills the model it is given, from its plan and base pointers ----
// rows layout: every dense pairwise factor becomes one row [table | m1 | m2] of a private buffer; its device offsets
// (relative to the const / dual base pointers, which the kernels add them to) point there from now on
static void layout_rows(ModelState& m, hipStream_t stream) {
  Plan& p = m.plan->p;
  std::vector<RowRec> rr;
  int64_t at = 0;
  for (int64_t f = 0; f < p.nf; ++f)
    if (p.f_kind[f] == LPMP_F_PAIRWISE_DENSE) {
      rr.push_back({p.f_doff[f], p.f_coff[f], at, p.f_dim0[f], p.f_dim1[f]});
      at += ((int64_t)p.f_dim0[f] * p.f_dim1[f] + p.f_dim0[f] + p.f_dim1[f] + 1) / 2 * 2;      // rows start 16-byte aligned
    }
  if (rr.empty()) return;
  m.d_rows.alloc((size_t)at);
  if ((((uintptr_t)m.d_rows.get() - (uintptr_t)m.d_const) % 16) != 0 || (((uintptr_t)m.d_rows.get() - (uintptr_t)m.d_dual) % 8) != 0)
    throw std::runtime_error("rows layout: buffers are not aligned to each other");
  m.d_rowrecs.alloc(rr.size());
  h2d(m.d_rowrecs, rr.data(), rr.size() * sizeof(RowRec), stream);
  m.n_rowrecs = (int64_t)rr.size();
  build_rows(m, stream);
  const int64_t c_shift = (int64_t)(((intptr_t)m.d_rows.get() - (intptr_t)m.d_const) / 8), d_shift = (int64_t)(((intptr_t)m.d_rows.get() - (intptr_t)m.d_dual) / 8);
  p.dev_coff.assign(p.f_coff.begin(), p.f_coff.end()); p.dev_doff.assign(p.f_doff.begin(), p.f_doff.end());
  size_t k = 0;
  for (int64_t f = 0; f < p.nf; ++f)
    if (p.f_kind[f] == LPMP_F_PAIRWISE_DENSE) {
      p.dev_coff[f] = c_shift + rr[k].row_off;
      p.dev_doff[f] = d_shift + rr[k].row_off + (int64_t)p.f_dim0[f] * p.f_dim1[f];
      ++k;
    }
  m.rows = true; m.packed_stale = false; m.rows_stale = false;
}
// SHARED pairwise factors: the host format is one double (the scale) per factor and a model-level pool of tables; on the
// device a factor's constants are two words {scale, offset of its table relative to the const base pointer} in an
// allocation of the engine's own, followed by the pool (always copied from the host: sh_data is host memory also when the
// packed constants are a device buffer of the caller's, which is why the scales are gathered by a kernel)
static void layout_shared_cells(ModelState& m, hipStream_t stream) {
  Plan& p = m.plan->p;
  std::vector<int64_t> sf;                      // the factor of every cell; a DIFF_SHIFT factor is listed twice (its two cells)
  for (int64_t f = 0; f < p.nf; ++f) {
    if (p.f_kind[f] == LPMP_F_PAIRWISE_SHARED || p.f_kind[f] == LPMP_F_PAIRWISE_DIFF) sf.push_back(f);   // (DIFF: the same two words, its vector D is a pool entry)
    else if (p.f_kind[f] == LPMP_F_PAIRWISE_DIFF_SHIFT) { sf.push_back(f); sf.push_back(f); }
  }
  // (the pool behind the cells: write_shared_pool)
  const int64_t n_sf = (int64_t)sf.size(), n_pool = p.sh_off[(size_t)p.n_shared] + p.n_shared;
  m.d_shared.alloc((size_t)(2 * n_sf + n_pool));
  if ((((uintptr_t)m.d_shared.get() - (uintptr_t)m.d_const) % 8) != 0) throw std::runtime_error("shared tables: buffers are not aligned to each other");
  const int64_t base = (int64_t)(((intptr_t)m.d_shared.get() - (intptr_t)m.d_const) / 8);
  std::vector<int64_t> cells((size_t)(2 * n_sf));
  if (p.dev_coff.empty()) p.dev_coff.assign(p.f_coff.begin(), p.f_coff.end());
  for (int64_t k = 0; k < n_sf; ++k) {
    const int64_t f = sf[(size_t)k];
    cells[(size_t)(2 * k)] = p.dev_coff[f];   // (the packed offset, or the factor's cell of the compact constants: table precision)
    cells[(size_t)(2 * k + 1)] = base + 2 * n_sf + shared_pool_at(p, p.f_table[f]);
    if (p.f_kind[f] == LPMP_F_PAIRWISE_DIFF_SHIFT) {   // its second cell: the shift, and n from the plan (structure: never from device memory)
      cells[(size_t)(2 * k + 2)] = p.dev_coff[f] + 1;
      cells[(size_t)(2 * k + 3)] = p.sh_dim1[(size_t)p.f_table[f]];
    }
    p.dev_coff[f] = base + 2 * k;
    if (p.f_kind[f] == LPMP_F_PAIRWISE_DIFF_SHIFT) ++k;
  }
  m.sh_cells = std::move(cells);
  write_shared_pool(m, stream, n_sf);
  gather_shared_cells(m, stream);
  std::vector<ShTableDesc> desc((size_t)p.n_shared);
  for (int t = 0; t < p.n_shared; ++t) desc[(size_t)t] = {base + 2 * n_sf + shared_pool_at(p, t), p.sh_dim0[(size_t)t], p.sh_dim1[(size_t)t]};
  m.d_sh_desc.alloc(desc.size());
  h2d(m.d_sh_desc, desc.data(), desc.size() * sizeof(ShTableDesc), stream);
}
// lower-bound records, in factor order, and runs of factors the streaming dense kernel can take; the tracked bounds start all NaN
static void layout_bound_records(ModelState& m, hipStream_t stream) {
  const Plan& p = m.plan->p;
  std::vector<LbRec> lb(p.nf);
  auto lb_class = [&](int64_t f) {
    if (p.f_kind[f] == LPMP_F_PAIRWISE_DENSE && p.f_dim0[f] == p.f_dim1[f] && (p.coff(f) % 2) == 0 &&
        (p.f_dim0[f] == 8 || p.f_dim0[f] == 16 || p.f_dim0[f] == 32)) return p.f_dim0[f];
    return 0;
  };
  for (int64_t f = 0; f < p.nf; ++f) {
    lb[f] = {p.doff(f), p.f_kind[f] == LPMP_F_VECTOR ? -1 : p.coff(f), p.f_dim0[f], p.f_dim1[f], p.f_kind[f] | (p.f_flags[f] << 4), 0};
    const int c = lb_class(f);
    if (m.lb_runs.empty() || m.lb_runs.back().cls != c) m.lb_runs.push_back({c, f, 1}); else m.lb_runs.back().count++;
  }
  m.d_lbrecs.alloc((size_t)p.nf);
  h2d(m.d_lbrecs, lb.data(), (size_t)p.nf * sizeof(LbRec), stream);
  m.d_lb.alloc((size_t)p.nf);
  m.d_part.alloc(1024);
  m.d_stale.alloc((size_t)p.nf);
  m.d_stale_n.alloc(1);
  HIP_CHECK(hipMemsetAsync(m.d_lb, 0xFF, (size_t)p.nf * sizeof(double), stream));   // all NaN: nothing tracked yet
  m.lb_all_stale = true;
}

// The model is built as a local value and committed by move at the very end: whatever throws on the way, the engine holds no
// model afterwards (the old one is dropped first: two models need not fit in device memory together).
int lpmp_upload_model(lpmp_engine* e, const lpmp_model* m, int const_mem, int dual_mem) {
  return guarded([&] {
    if (!e || !m) throw std::runtime_error("null argument");
    HIP_CHECK(hipSetDevice(e->device));
    if (e->model.plan && !e->model.own_dual() && e->model.batch.n > 0) settle(e);   // the caller keeps the old model's (borrowed) dual buffer: leave it at the caller's pass
    HIP_CHECK(hipStreamSynchronize(e->stream));
    e->release_model();   // (an open speculative batch in an engine-owned buffer dies with the old model)
    ModelState next;
    next.plan = std::make_unique<lpmp_plan>();
    Plan& p = next.plan->p;
    p.build(*m);
    const int64_t n_const = p.f_coff[p.nf], n_dual = p.f_doff[p.nf];
    if ((n_const > 0 && !m->const_data) || !m->dual_data) throw std::runtime_error("cost arrays missing");
    // streamed-once access policy (kernels.hip, ld_stream): only when the state cannot live in the 256 MiB Infinity Cache
    {
      const char* env = getenv("LPMP_NT");
      const bool big = (n_const + n_dual) * (int64_t)sizeof(double) > (int64_t)1 << 30;
      next.nt_flag = (env ? atoi(env) != 0 : big) ? SWEEP_NT : 0;
      next.model_big = big;
    }
    const bool f32 = e->want_tab != LPMP_TABLES_F64;
    if (f32 && e->want_rows) throw UnsupportedError("table precision f32 and the rows layout cannot be combined (the rows hold the tables as doubles)");
    if (f32) { p.tables_f32 = true; next.tab_prec = e->want_tab; next.tab_flag = SWEEP_TAB32; }   // before the first schedule: the byte accounting of every plan of this model
    if (const_mem == LPMP_MEM_DEVICE) {
      next.d_const = const_cast<double*>(m->const_data);
      if (((uintptr_t)next.d_const & 15) != 0) throw std::runtime_error("device const buffer must be 16-byte aligned");
      if (f32) narrow_tables(next, e->stream, m->const_data, true);
    } else if (f32) {
      next.tab_compact = true;
      narrow_tables(next, e->stream, m->const_data, false);
    } else if (n_const > 0) {
      next.const_buf.alloc((size_t)n_const);
      next.d_const = next.const_buf;
      h2d(next.d_const, m->const_data, (size_t)n_const * sizeof(double), e->stream);
    }
    if (dual_mem == LPMP_MEM_DEVICE) {
      next.d_dual = const_cast<double*>(m->dual_data);
    } else {
      next.dual_buf.alloc((size_t)n_dual);
      next.d_dual = next.dual_buf;
      h2d(next.d_dual, m->dual_data, (size_t)n_dual * sizeof(double), e->stream);
    }
    if (e->want_rows && next.d_const) layout_rows(next, e->stream);
    if (!p.f_table.empty()) layout_shared_cells(next, e->stream);
    if (!p.tab_data.empty()) {
      next.d_tabs.alloc(p.tab_data.size());
      h2d(next.d_tabs, p.tab_data.data(), p.tab_data.size() * sizeof(int32_t), e->stream);
    }
    layout_bound_records(next, e->stream);
    if (!e->pinned) {
      e->pinned = pinned_pool().take();
      e->h_part = (double*)e->pinned;                               // [0, 1024) doubles: partial sums
      e->h_stale_n = (unsigned long long*)(e->pinned + 8 * 1024);   // one counter
      e->h_pbad = (int*)(e->pinned + 8 * 1024 + 64);                // one flag
    }
    HIP_CHECK(hipStreamSynchronize(e->stream));
    { static std::atomic<uint64_t> gen{0}; next.model_gen = ++gen; }   // (read-outs of an earlier model answer LPMP_ERR_STATE from here on)
    p.force_generic = e->rtype == LPMP_RTYPE_ADAPTIVE;
    {   // mailbox budget of every schedule planned for this model: half of what the device has left now (LPMP_MAILBOX_MB overrides)
      size_t free_b = 0, total_b = 0;
      if (const char* v = std::getenv("LPMP_MAILBOX_MB")) p.mailbox_budget_bytes = (int64_t)std::atoll(v) << 20;
      else if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) p.mailbox_budget_bytes = (int64_t)(free_b / 2);
      else (void)hipGetLastError();
    }
    check_rtype(next, e->rtype);
    e->model = std::move(next);
  });
}

int lpmp_set_reparametrization(lpmp_engine* e, int mode) {
  return guarded([&] {
    require_model(e);
    if (mode == LPMP_REPAM_MIXED) throw UnsupportedError("mixed reparametrization is assert(false) in the reference (LP_MP.h:1455)");
    if (mode < 0 || mode >= LPMP_REPAM_COUNT) throw std::runtime_error("unknown reparametrization mode");
    HIP_CHECK(hipSetDevice(e->device));
    if (mode != e->model.mode) settle(e);          // (Solver::PreIterate sets the same mode before every pass, solver.hxx:268-271)
    // The directional schedules (ComputeForwardPass / ComputeBackwardPass, the ...AndPrimal sweeps) are built here for models of
    // ordinary size — a model the device kernels cannot run is refused at this call — and on first use for models of millions of
    // factors: LP::ComputePass runs the fused pass schedule and the partitioned drivers their own iterator-range schedules, and
    // two directional schedules nobody runs were 2.6 s of the 10 s before the first pass of the 2 M / 10 M graph
    if (e->model.plan->p.nf <= LAZY_SCHEDULES_MIN_FACTORS) ensure_device_schedules(e, mode);
    else e->model.plan->p.ensure_weights(mode);
    e->model.mode = mode;
  });
}

static void apply_rtype(lpmp_engine* e, int rtype) {
  const bool generic = rtype == LPMP_RTYPE_ADAPTIVE;
  if (e->model.plan && e->model.plan->p.force_generic != generic) {   // other kernel classes: every built-in schedule is rebuilt
    e->model.release_schedules();
    e->model.plan->drop_caches();
    e->model.plan->p.force_generic = generic;
    e->model.mode = -1;
  }
  e->rtype = rtype;
}

int lpmp_set_reparametrization_type(lpmp_engine* e, int rtype) {
  return guarded([&] {
    if (!e) throw std::runtime_error("null engine");
    if (rtype < LPMP_RTYPE_SHARED || rtype > LPMP_RTYPE_ADAPTIVE) throw std::runtime_error("unknown reparametrization type");
    check_rtype(e->model, rtype);
    if (rtype != e->rtype) settle(e);
    if (rtype != e->rtype) {   // captured graphs bake the kernel flag in
      HIP_CHECK(hipStreamSynchronize(e->stream));
      for (int d = 0; d < 2; ++d) for (int m = 0; m < LPMP_REPAM_COUNT; ++m)
        e->model.sched[d][m].graph.reset();
      for (int m = 0; m < LPMP_REPAM_COUNT; ++m)
        e->model.sched_pass[m].graph.reset();
      for (int k = 0; k < 2; ++k) e->model.sched_part[k].graph.reset();
      for (auto& c : e->model.custom) if (c) c->graph.reset();
    }
    const int mode = e->model.mode;
    apply_rtype(e, rtype);
    if (e->model.mode < 0 && mode >= 0) { ensure_device_schedules(e, mode); e->model.mode = mode; }   // the mode survives the rebuild
  });
}

int lpmp_set_inner_iterations(lpmp_engine* e, int n) {
  return guarded([&] {
    if (!e) throw std::runtime_error("null engine");
    if (n < 1) throw std::runtime_error("innerIteration must be positive");
    if (n != e->inner_iterations) {
      settle(e);
      HIP_CHECK(hipStreamSynchronize(e->stream));
      for (int k = 0; k < 2; ++k) { e->model.sched_part[k].release(); e->model.have_part[k] = false; }
    }
    e->inner_iterations = n;
  });
}

// compute_partition_pass / compute_overlapping_partition_pass (reference LP_MP.h:1932-2051): a fixed sequence of
// iterator-range passes over the partitions' factor lists with their own anisotropic weights.  The whole sequence is
// level-scheduled as ONE schedule: inner iterations of partitions that touch no common factor run side by side.
static void ensure_partition_schedule(lpmp_engine* e, int rtype) {
  const int k = rtype - LPMP_RTYPE_PARTITION;
  if (e->model.have_part[k]) return;
  std::vector<Plan::Segment> segs;
  e->model.plan->p.partition_pass_segments(rtype, e->inner_iterations, segs);
  Schedule s;
  e->model.plan->p.make_schedule(segs, e->use_fused, s);
  check_generic_limits(e->model.plan->p, s);
  upload_schedule(e, s, e->model.sched_part[k]);
  e->model.have_part[k] = true;
}

int lpmp_compute_forward_pass(lpmp_engine* e) {
  return guarded([&] { require_mode(e); HIP_CHECK(hipSetDevice(e->device)); settle(e); ensure_device_schedules(e, e->model.mode); begin_compute(e); run_schedule(e, e->model.sched[0][e->model.mode]); });
}
int lpmp_compute_backward_pass(lpmp_engine* e) {
  return guarded([&] { require_mode(e); HIP_CHECK(hipSetDevice(e->device)); settle(e); ensure_device_schedules(e, e->model.mode); begin_compute(e); run_schedule(e, e->model.sched[1][e->model.mode]); });
}
static void compute_plain_passes(lpmp_engine* e, int n) {   // ComputeForwardPass(); ComputeBackwardPass(); n times
  if (e->use_fused) {
    ensure_pass_schedule(e, e->model.mode);
    if (e->model.rotation_ok[e->model.mode] && e->use_rotation) {
      // passes in slices of at most 32: each slice one persistent launch (memory of the ticket arrays stays bounded)
      int done = 0;
      while (done < n) {
        const int m = std::min(n - done, 32);
        if (!run_rotation_chain(e, e->model.mode, m)) break;
        done += m;
      }
      if (done == n) return;
      n -= done;
    }
    if (n >= 2 && e->model.rotation_ok[e->model.mode] && e->use_rotation) {
      const LaunchView fb = e->model.sched_pass[e->model.mode].view(), bf = e->model.sched_bf[e->model.mode].view();
      const bool timed = e->timing;
      issue_launches(e, fb, timed, e->stream, 1);
      issue_launches(e, fb, timed, e->stream, 2);
      for (int i = 1; i < n; ++i) { issue_launches(e, bf, timed, e->stream, 2); issue_launches(e, fb, timed, e->stream, 2); }
      issue_launches(e, fb, timed, e->stream, 3);
      if (timed && e->pending.size() > 4096) e->drain_timing();
    } else {
      ensure_pass_chain_plan(e, e->model.mode);
      for (int i = 0; i < n; ++i) run_schedule(e, e->model.sched_pass[e->model.mode]);
    }
  } else {
    ensure_device_schedules(e, e->model.mode);
    for (int i = 0; i < n; ++i) { run_schedule(e, e->model.sched[0][e->model.mode]); run_schedule(e, e->model.sched[1][e->model.mode]); }
  }
}
// build whatever lpmp_compute_pass(e, n) needs that depends on n (the ticket order of n joined passes), outside of a
// timed region; optional
int lpmp_prepare_passes(lpmp_engine* e, int n) {
  return guarded([&] {
    require_mode(e);
    if (n < 1) throw std::runtime_error("bad argument");
    HIP_CHECK(hipSetDevice(e->device));
    if (e->rtype != LPMP_RTYPE_SHARED || !e->use_fused) return;
    ensure_pass_schedule(e, e->model.mode);
    if (!(e->model.rotation_ok[e->model.mode] && e->use_rotation && e->use_chain && e->use_blocked_passes)) return;
    for (int done = 0; done < n;) { const int m = std::min(n - done, 32); (void)rotation_chain(e, e->model.mode, m); done += m; }
  });
}
// ---- speculative passes ---------------------------------------------------------------------------------------------
// The reference's caller asks for ONE pass per iteration and, by default, for the bound after every pass
// (Solver::Iterate / PostIterate, solver.hxx:273-284), while the device is fastest when consecutive passes are ONE
// persistent launch in Infinity-Cache order (rotation_chain: 5.1 against 6.6 ms per pass on C3).  With speculation on,
// lpmp_compute_pass(e, 1) launches a BATCH of n passes ahead of the caller — after a snapshot of the duals — and the
// launch itself leaves the tracked bounds of all factors as they are at the end of every pass (one row per pass,
// kernels.hpp HIST_END / HIST_MID).  The following n - 1 calls of lpmp_compute_pass(e, 1) only advance a cursor, and
// lpmp_lower_bound returns the bound of the pass the caller is at (the sum of that row, in the order lpmp_lower_bound sums).
// ANY other call settles first: if the caller stopped inside the batch the duals go back to the snapshot and exactly the
// passes it asked for are run again (bit-identical: n joined passes equal n single ones).  So the speculation
// is invisible except in time; how far ahead is learnt from the caller: batches double while single passes keep coming
// and restart at the length of the previous run (MpRoundingSolver: four plain passes between two rounding iterations).
static void spec_interrupt(lpmp_engine* e) {
  auto& sp = e->model.batch;
  if (sp.run_len > 0) sp.learned = sp.run_len;
  sp.run_len = 0; sp.last_batch = 0;
}
void settle(lpmp_engine* e) {
  if (!e) return;
  auto& sp = e->model.batch;
  if (sp.n > 0) {
    const int n = sp.n, pos = sp.pos;
    sp.n = 0; sp.pos = 0; sp.lb_ready = false;
    if (pos < n && e->model.plan) {   // the caller stopped inside the batch: back to its start, then exactly the passes it asked for
      HIP_CHECK(hipSetDevice(e->device));
      const size_t nd = (size_t)e->model.plan->p.f_doff[e->model.plan->p.nf], nf = (size_t)e->model.plan->p.nf;
      HIP_CHECK(hipMemcpyAsync(e->model.d_dual, sp.d_snap, nd * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      HIP_CHECK(hipMemcpyAsync(e->model.d_lb, sp.d_snap + nd, nf * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      e->model.lb_all_stale = sp.snap_lb_stale;
      ++e->spec.rollbacks;
      const int mode = e->model.mode;
      e->model.mode = sp.mode;          // (set_reparametrization settles before it changes the mode)
      try { compute_plain_passes(e, pos); } catch (...) { e->model.mode = mode; throw; }
      e->model.mode = mode;
    }
  }
  spec_interrupt(e);
}
static void lb_sum_blocks(int64_t nf, int64_t& nb, int64_t& per) {   // the partition lpmp_lower_bound sums in
  nb = std::min<int64_t>(1024, (nf + 255) / 256);
  per = (nf + nb - 1) / nb;
  nb = (nf + per - 1) / per;
}
static bool spec_start_batch(lpmp_engine* e, int depth) {
  auto& sp = e->model.batch;
  ensure_pass_schedule(e, e->model.mode);
  // (the bound rows are written by the dense chain body only: kernels.hip, dense_pk_body)
  if (!(e->model.rotation_ok[e->model.mode] && e->model.plan->rot[e->model.mode].valid && e->model.plan->rot[e->model.mode].hist_ok && kc_is_dense(e->model.plan->rot[e->model.mode].kclass))) return false;
  depth = std::min(depth, 32);
  if (!rotation_chain(e, e->model.mode, depth)) return false;
  const size_t nd = (size_t)e->model.plan->p.f_doff[e->model.plan->p.nf], nf = (size_t)e->model.plan->p.nf;
  // (an allocation that fails switches speculation OFF for this engine — the plain pass needs none of these buffers — instead
  // of making every lpmp_compute_pass(e, 1) fail on a model that solves fine without: snapshot = all duals + tracked bounds)
  auto grow = [&](DevBuf<double>& b, size_t want) -> bool {
    if (want <= b.capacity()) return true;
    HIP_CHECK(hipStreamSynchronize(e->stream));
    return b.try_alloc(want);
  };
  if (!grow(sp.d_snap, nd + nf) || !grow(sp.d_hist, (size_t)(std::min(e->spec.max_depth, 32) - 1) * nf) ||
      !grow(sp.d_hpart, (size_t)(std::min(e->spec.max_depth, 32) - 1) * 1024)) {
    sp = SpecBatch();
    e->spec.max_depth = 0;
    ++e->spec.alloc_failures;
    return false;
  }
  HIP_CHECK(hipMemcpyAsync(sp.d_snap, e->model.d_dual, nd * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  HIP_CHECK(hipMemcpyAsync(sp.d_snap + nd, e->model.d_lb, nf * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  sp.snap_lb_stale = e->model.lb_all_stale;
  if (!run_rotation_chain(e, e->model.mode, depth, sp.d_hist)) return false;
  // the device is `depth` passes ahead from here on: the batch is open BEFORE anything else can fail, so that settle() rolls back
  sp.n = depth; sp.pos = 0; sp.mode = e->model.mode; sp.lb_ready = false; sp.last_batch = depth;
  ++e->spec.batches; e->spec.passes_launched += depth;
  int64_t nb, per; lb_sum_blocks((int64_t)nf, nb, per);
  for (int i = 0; i < depth - 1; ++i) launch_sum_stage(sp.d_hist + (size_t)i * nf, sp.d_hpart + (size_t)i * 1024, (int64_t)nf, per, nb, e->stream);
  HIP_CHECK(hipGetLastError());
  return true;
}
// the bound of the pass the caller is at, while that pass lies inside an open batch
static bool spec_lower_bound(lpmp_engine* e, double* out) {
  auto& sp = e->model.batch;
  if (!(sp.n > 0 && sp.pos < sp.n)) return false;
  if (!sp.lb_ready) {
    check_chain(e);
    const int64_t nf = e->model.plan->p.nf;
    int64_t nb, per; lb_sum_blocks(nf, nb, per);
    std::vector<double> h((size_t)(sp.n - 1) * 1024);
    d2h(h.data(), sp.d_hpart, h.size() * sizeof(double), e->stream);
    sp.lb.assign((size_t)sp.n - 1, 0.0);
    for (int i = 0; i < sp.n - 1; ++i) {
      double lb = e->model.plan->p.constant;
      for (int64_t j = 0; j < nb; ++j) lb += h[(size_t)i * 1024 + j];
      sp.lb[i] = lb;
    }
    sp.lb_ready = true;
  }
  *out = sp.lb[sp.pos - 1];
  return true;
}
static bool spec_usable(const lpmp_engine* e) {
  return e->spec.max_depth >= 2 && e->rtype == LPMP_RTYPE_SHARED && e->use_fused && e->use_rotation && e->use_chain &&
         e->use_blocked_passes && e->use_lb_tracking && !e->timing && !e->model.rows;
}

int lpmp_set_speculation(lpmp_engine* e, int max_passes_ahead) {
  return guarded([&] {
    if (!e) throw std::runtime_error("null engine");
    if (max_passes_ahead < 0) throw std::runtime_error("bad argument");
    settle(e);
    e->spec.max_depth = std::min(max_passes_ahead, 32);
    if (e->spec.max_depth < 2) { HIP_CHECK(hipStreamSynchronize(e->stream)); e->model.batch = SpecBatch(); }
  });
}
int lpmp_speculation_stats(lpmp_engine* e, int64_t* batches, int64_t* passes_launched, int64_t* passes_used, int64_t* rollbacks) {
  return guarded([&] {
    if (!e) throw std::runtime_error("null engine");
    if (batches) *batches = e->spec.batches;
    if (passes_launched) *passes_launched = e->spec.passes_launched;
    if (passes_used) *passes_used = e->spec.passes_used;
    if (rollbacks) *rollbacks = e->spec.rollbacks;
  });
}
int64_t lpmp_chain_cache_bytes(const lpmp_engine* e) { return e ? (int64_t)e->model.rot_cache_bytes : 0; }

int lpmp_compute_pass(lpmp_engine* e, int n) {   // LP::ComputePass, LP_MP.h:869-887
  return guarded([&] {
    require_mode(e);
    HIP_CHECK(hipSetDevice(e->device));
    begin_compute(e);
    if (n == 1 && e->spec.max_depth >= 2) {
      auto& sp = e->model.batch;
      if (sp.n > 0) {
        if (sp.pos < sp.n) { ++sp.pos; ++sp.run_len; ++e->spec.passes_used; return; }   // already on its way
        sp.n = 0; sp.pos = 0; sp.lb_ready = false;                                  // used up: the device state is the caller's
      }
      if (spec_usable(e)) {
        int depth = sp.run_len == 0 ? (sp.learned > 0 ? sp.learned : 2) : std::max(2, 2 * sp.last_batch);
        depth = std::min(depth, e->spec.max_depth);
        if (depth >= 2 && spec_start_batch(e, depth)) { sp.pos = 1; ++sp.run_len; ++e->spec.passes_used; return; }
      }
      ++sp.run_len; sp.last_batch = 0;
      if (e->rtype == LPMP_RTYPE_SHARED) { compute_plain_passes(e, 1); return; }
    } else settle(e);
    if (e->rtype == LPMP_RTYPE_PARTITION) {
      ensure_partition_schedule(e, e->rtype);
      for (int i = 0; i < n; ++i) run_schedule(e, e->model.sched_part[0]);
    } else if (e->rtype == LPMP_RTYPE_OVERLAPPING_PARTITION) {
      ensure_partition_schedule(e, e->rtype);
      for (int i = 0; i < n; ++i) { run_schedule(e, e->model.sched_part[1]); compute_plain_passes(e, 1); }
    } else {
      compute_plain_passes(e, n);
    }
  });
}

// ---- primal rounding inside the sweep ------------------------------------------------------------------------------
// What the reference does per updated factor (UpdateFactorPrimal) is split in three: the lazy init of everything the
// pass touches (one kernel, only when the time stamp grows — all touched factors carry the same stamp), the label of
// every COMPUTE_PRIMAL unary inside the sweep kernels (state after its receives), and the copy of the labels into the
// pairwise factors afterwards.  The copy can wait because a pairwise factor's primal_[side] has a single writer and
// nothing reads it before EvaluatePrimal: with a `left` schedule the recursion of propagate_primal_through_messages
// stops at the pairwise factor (its other side is unset or already equal).
// init_primal of every factor: an unset entry holds the dimension (what PrimalInit records say for the touched ones)
void upload_unset_primal(lpmp_engine* e) {
  const Plan& p = e->model.plan->p;
  if (p.nf <= 0) return;
  std::vector<int32_t> h(2 * (size_t)p.nf);
  for (int64_t f = 0; f < p.nf; ++f) { h[2 * f] = p.f_dim0[f]; h[2 * f + 1] = p.f_kind[f] == LPMP_F_VECTOR ? 0 : p.f_dim1[f]; }
  h2d(e->model.d_primal, h.data(), h.size() * sizeof(int32_t), e->stream);
}
void ensure_primal(lpmp_engine* e) {
  if (e->model.have_primal) return;
  // (every refusal below comes before anything is released or allocated: on a model this code refuses, the array of unset labels
  // that lpmp_path_moves / lpmp_forest_moves / lpmp_readout_labels keep — primal_unset_only — survives the refused call)
  const Plan& p = e->model.plan->p;
  for (const auto& mt : p.mtypes)
    if (mt.kind != LPMP_M_UNARY_PAIRWISE)
      throw UnsupportedError("primal rounding is built for unary / pairwise models (DESIGN.md 8)");
  // Pairwise factor types with COMPUTE_PRIMAL_SOLUTION (MPLP-style `right` / `full` schedules): the recursion of
  // propagate_primal_through_messages then runs pairwise -> its unaries -> their other pairwise factors and stops
  // (a slot that is set always equals its unary's label, so nothing changes further out).  The device keeps the
  // UNARY labels as the one source of truth inside a sweep: an updated pairwise factor of such a type reads its
  // sides from its unaries' labels, fills the free ones (first minimiser in row-major order given the others) and
  // labels those unaries; the pairwise slots are copies, made after the sweep as before.  Such records run on the
  // generic kernels in primal passes (issue_launches) and depend on all their unaries (plan.cpp, make_schedule).
  bool pw_computes = false;
  for (int64_t f = 0; f < p.nf; ++f) if (p.f_kind[f] != LPMP_F_VECTOR && p.ftype_primal[p.f_type[f]] && p.updated[f]) pw_computes = true;
  std::vector<PrimalLink> prop, rest;
  std::vector<int32_t> writer(2 * (size_t)p.nf, -1);
  std::vector<uint8_t> touched((size_t)p.nf, 0), labelable((size_t)p.nf, 0);
  for (int64_t m = 0; m < p.nm; ++m) {
    const int32_t l = p.m_left[m], r = p.m_right[m];
    if (p.f_kind[l] != LPMP_F_VECTOR || p.f_kind[r] == LPMP_F_VECTOR) throw UnsupportedError("primal rounding: unary-pairwise message between unexpected factor kinds");
    if (p.ftype_primal[p.f_type[l]] || (p.ftype_primal[p.f_type[r]] && p.updated[r])) labelable[l] = 1;
  }
  for (int64_t m = 0; m < p.nm; ++m) {
    const int32_t l = p.m_left[m], r = p.m_right[m];
    const int side = p.mtypes[p.m_type[m]].param;
    const PrimalLink k{l, r, side, p.f_dim0[l]};
    if (labelable[l]) {
      int32_t& w = writer[2 * (size_t)r + side];   // the copy into the pairwise factor is deferred: one writer per slot
      if (w >= 0 && w != l) throw UnsupportedError("primal rounding: two unaries on one side of a pairwise factor");
      w = l;
      prop.push_back(k);
      touched[r] = 1;
    } else rest.push_back(k);
  }
  e->model.release_primal();   // a previous attempt may have stopped half way
  if (pw_computes) {
    // conditionally_init_primal reaches one step further: a pairwise factor whose slot changes initialises all its unaries
    for (int64_t m = 0; m < p.nm; ++m) if (touched[p.m_right[m]]) touched[p.m_left[m]] = 2;
    std::vector<int32_t> h(2 * (size_t)p.nf);
    for (size_t i = 0; i < h.size(); ++i) h[i] = writer[i];
    e->model.d_pw_unary.alloc(std::max<size_t>(1, h.size()));
    if (!h.empty()) h2d(e->model.d_pw_unary, h.data(), h.size() * sizeof(int32_t), e->stream);
  }
  for (int64_t f = 0; f < p.nf; ++f) if (p.updated[f]) touched[f] = 1;
  auto unset = [&](int64_t f) { return PrimalInit{(int32_t)f, p.f_dim0[f], p.f_kind[f] == LPMP_F_VECTOR ? 0 : p.f_dim1[f], 0}; };
  std::vector<PrimalInit> init;
  for (int64_t f = 0; f < p.nf; ++f) if (touched[f]) init.push_back(unset(f));
  e->model.n_pprop = (int64_t)prop.size();
  prop.insert(prop.end(), rest.begin(), rest.end());
  e->model.n_plinks = (int64_t)prop.size();
  e->model.n_pinit = (int64_t)init.size();
  e->model.d_primal.alloc(std::max<size_t>(1, 2 * (size_t)p.nf));
  e->model.d_pcost.alloc(std::max<size_t>(1, (size_t)p.nf));
  e->model.d_pbad.alloc(1);
  if (!prop.empty()) {
    e->model.d_plinks.alloc(prop.size());
    h2d(e->model.d_plinks, prop.data(), prop.size() * sizeof(PrimalLink), e->stream);
  }
  // every factor starts unset (init_primal), then only the touched ones are ever re-initialised
  upload_unset_primal(e);
  if (!init.empty()) {
    e->model.d_pinit.alloc(init.size());
    h2d(e->model.d_pinit, init.data(), init.size() * sizeof(PrimalInit), e->stream);
  }
  e->model.primal_t = 0;
  e->model.have_primal = true;
}
// the primal array of a call that reads or writes labels on any model: the one ensure_primal makes, or, on a model the rounding code
// does not take (messages other than unary-pairwise), the array of unset labels in which only unaries ever get a label.  That array
// is made once and remembered until release_primal (the model goes); a refused call leaves it (ensure_primal)
void ensure_label_array(lpmp_engine* e) {
  ModelState& m = e->model;
  if (m.have_primal || m.primal_unset_only) return;
  try { ensure_primal(e); }
  catch (const UnsupportedError&) {
    m.d_primal.alloc(std::max<size_t>(1, 2 * (size_t)m.plan->p.nf));
    upload_unset_primal(e);
    m.primal_unset_only = true;
  }
}

static void run_primal_sweep(lpmp_engine* e, int d, uint64_t t) {
  require_mode(e);
  HIP_CHECK(hipSetDevice(e->device));
  settle(e);
  begin_compute(e);
  ensure_primal(e);
  // the reference asserts primal_access_ <= timestamp (factors_messages.hxx:3304); in a release build a smaller
  // stamp lowers primal_access_ of the rounded factors only and later passes depend on the update order
  if (t < e->model.primal_t) throw std::runtime_error("primal pass: time stamps (2*iteration+1 / +2) must not decrease");
  if (t > e->model.primal_t) {   // conditionally_init_primal: primal_access_ < timestamp
    launch_primal_init(e->model.d_pinit, e->model.n_pinit, e->model.d_primal, e->stream);
    e->model.primal_t = t;
  }
  ensure_device_schedules(e, e->model.mode);
  e->primal_pass = true;
  try { run_schedule(e, e->model.sched[d][e->model.mode]); } catch (...) { e->primal_pass = false; throw; }
  e->primal_pass = false;
  launch_primal_propagate(e->model.d_plinks, e->model.n_pprop, e->model.d_primal, e->stream);
  HIP_CHECK(hipGetLastError());
}

int lpmp_compute_forward_pass_and_primal(lpmp_engine* e, uint64_t iteration) {
  return guarded([&] { run_primal_sweep(e, 0, 2 * iteration + 1); });
}
int lpmp_compute_backward_pass_and_primal(lpmp_engine* e, uint64_t iteration) {
  return guarded([&] { run_primal_sweep(e, 1, 2 * iteration + 2); });
}
int lpmp_compute_pass_and_primal(lpmp_engine* e, uint64_t iteration) {
  return guarded([&] { run_primal_sweep(e, 0, 2 * iteration + 1); run_primal_sweep(e, 1, 2 * iteration + 2); });
}

static bool primal_consistent(lpmp_engine* e) {
  HIP_CHECK(hipMemsetAsync(e->model.d_pbad, 0, sizeof(int), e->stream));
  launch_primal_check(e->model.d_plinks, e->model.n_plinks, e->model.d_primal, e->model.d_pbad, e->stream);
  HIP_CHECK(hipMemcpyAsync(e->h_pbad, e->model.d_pbad, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
  return *e->h_pbad == 0;
}
int lpmp_check_primal_consistency(lpmp_engine* e, int* consistent) {
  return guarded([&] {
    require_model(e);
    if (!consistent) throw std::runtime_error("null argument");
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);
    ensure_primal(e);
    *consistent = primal_consistent(e) ? 1 : 0;
  });
}
int lpmp_evaluate_primal(lpmp_engine* e, double* cost) {
  return guarded([&] {
    require_model(e);
    if (!cost) throw std::runtime_error("null argument");
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);
    require_consts(e);
    ensure_primal(e);
    if (!primal_consistent(e)) { *cost = std::numeric_limits<double>::infinity(); return; }
    const int64_t nf = e->model.plan->p.nf;
    rows_refresh(e);
    launch_primal_cost(e->model.d_lbrecs, e->model.d_dual, e->model.d_const, e->model.d_primal, e->model.d_pcost, nf, e->model.tab_flag, e->stream);
    int64_t nb = std::min<int64_t>(1024, (nf + 255) / 256);
    const int64_t per = (nf + nb - 1) / nb;
    nb = (nf + per - 1) / per;
    launch_sum_stage(e->model.d_pcost, e->model.d_part, nf, per, nb, e->stream);
    HIP_CHECK(hipMemcpyAsync(e->h_part, e->model.d_part, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_CHECK(hipStreamSynchronize(e->stream));
    double c = e->model.plan->p.constant;
    for (int64_t i = 0; i < nb; ++i) c += e->h_part[i];
    *cost = c;
  });
}
// the same value into the caller's device memory: no host synchronisation, no device-to-host copy.  The last kernel reads the
// consistency flag and adds the partial sums as the host does above
int lpmp_evaluate_primal_dev(lpmp_engine* e, double* dst_dev) {
  return guarded([&] {
    require_model(e);
    if (!dst_dev) throw std::runtime_error("lpmp_evaluate_primal_dev: null destination");
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);
    require_consts(e);
    ensure_primal(e);
    ModelState& m = e->model;
    const int64_t nf = m.plan->p.nf;
    HIP_CHECK(hipMemsetAsync(m.d_pbad, 0, sizeof(int), e->stream));
    launch_primal_check(m.d_plinks, m.n_plinks, m.d_primal, m.d_pbad, e->stream);
    rows_refresh(e);
    launch_primal_cost(m.d_lbrecs, m.d_dual, m.d_const, m.d_primal, m.d_pcost, nf, m.tab_flag, e->stream);
    int64_t nb, per; lb_sum_blocks(nf, nb, per);
    launch_sum_stage(m.d_pcost, m.d_part, nf, per, nb, e->stream);
    launch_sum_final(m.d_part, nb, m.plan->p.constant, m.d_pbad, dst_dev, e->stream);
    HIP_CHECK(hipGetLastError());
  });
}
int lpmp_download_primal(lpmp_engine* e, int32_t* out) {
  return guarded([&] {
    require_model(e);
    if (!out) throw std::runtime_error("null argument");
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);
    ensure_primal(e);
    d2h(out, e->model.d_primal, 2 * (size_t)e->model.plan->p.nf * sizeof(int32_t), e->stream);
  });
}
int lpmp_upload_primal(lpmp_engine* e, const int32_t* in) {
  return guarded([&] {
    require_model(e);
    if (!in) throw std::runtime_error("null argument");
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);
    ensure_primal(e);
    h2d(e->model.d_primal, in, 2 * (size_t)e->model.plan->p.nf * sizeof(int32_t), e->stream);
  });
}

// ---- conditional rounding from the duals -------------------------------------------------------------------
// The device tables of a direction: the planner's unaries sorted by (level, class) — class 0: at most DECODE_GROUP_MAX labels, a
// lane group per unary; class 1: a wave per unary — with the device offsets of the uploaded model (rows layout, float tables and
// SHARED / DIFF cells are all behind Plan::doff / coff).  A function of the structure, like a schedule, and counted as one.
static void ensure_decode(lpmp_engine* e, int d) {
  DevDecode& dd = e->model.decode[d];
  if (dd.have) return;
  dd.release();
  const DecodePlan& dp = decode_plan_or_refuse(e->model.plan.get(), d);
  const Plan& p = e->model.plan->p;
  const size_t nu = dp.unaries.size();
  auto bucket = [&](size_t i) { return 2 * (size_t)(dp.level[i] - 1) + (p.f_dim0[dp.unaries[i]] > DECODE_GROUP_MAX ? 1 : 0); };
  std::vector<int64_t> start(2 * (size_t)dp.n_levels + 1, 0);
  std::vector<int32_t> width(2 * (size_t)dp.n_levels, 0);
  for (size_t i = 0; i < nu; ++i) { const size_t b = bucket(i); ++start[b + 1]; width[b] = std::max(width[b], p.f_dim0[dp.unaries[i]]); }
  for (size_t b = 0; b + 1 < start.size(); ++b) start[b + 1] += start[b];
  std::vector<int32_t> level_of((size_t)p.nf, 0);
  for (size_t i = 0; i < nu; ++i) level_of[(size_t)dp.unaries[i]] = dp.level[i];
  std::vector<DecodeRec> recs(nu);
  std::vector<DecodeLink> links(dp.edges.size());
  {
    std::vector<int64_t> cur(start.begin(), start.end() - 1);
    for (size_t i = 0; i < nu; ++i) {
      const int32_t u = dp.unaries[i];
      recs[(size_t)cur[bucket(i)]++] = {p.doff(u), p.f_dim0[u], (int32_t)dp.edge_off[i], (int32_t)(dp.edge_off[i + 1] - dp.edge_off[i]), u};
    }
  }
  for (size_t k = 0; k < links.size(); ++k) {
    const DecodeEdge& ed = dp.edges[k];
    links[k] = {p.doff(ed.p), p.coff(ed.p), p.f_kind[ed.p], p.f_dim0[ed.p], p.f_dim1[ed.p], ed.side, ed.other, level_of[(size_t)ed.other]};
  }
  for (size_t b = 0; b + 1 < start.size(); ++b)
    if (start[b + 1] > start[b]) dd.launches.push_back({start[b], start[b + 1] - start[b], width[b], (int32_t)(b / 2) + 1});
  if (nu) { dd.recs.alloc(nu); h2d(dd.recs, recs.data(), nu * sizeof(DecodeRec), e->stream); }
  if (!links.empty()) { dd.links.alloc(links.size()); h2d(dd.links, links.data(), links.size() * sizeof(DecodeLink), e->stream); }
  dd.have = true;
  ++e->model.schedules_built;
  deep_schedule_note(e, dp.n_levels, "the decode order");
}

int lpmp_decode_primal(lpmp_engine* e, int direction, int refine_sweeps) {
  return guarded([&] {
    require_model(e);
    if (direction < 0 || direction > 1) throw std::runtime_error("lpmp_decode_primal: direction must be LPMP_FORWARD or LPMP_BACKWARD");
    if (refine_sweeps < 0) throw std::runtime_error("lpmp_decode_primal: negative number of refinement sweeps");
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);                 // passes that ran ahead: the duals decoded are those of the pass the caller is at
    require_consts(e);
    ensure_decode(e, direction);
    ensure_primal(e);
    rows_refresh(e);           // (reads the rows; writes no dual)
    const DevDecode& dd = e->model.decode[direction];
    for (int sweep = 0; sweep <= refine_sweeps; ++sweep)
      for (const auto& l : dd.launches)
        launch_decode(dd.recs, dd.links, e->model.d_dual, e->model.d_const, e->model.d_primal, l.first, l.count, l.width, l.level, sweep ? DECODE_ALL : 0, e->model.tab_flag, e->stream);
    launch_primal_propagate(e->model.d_plinks, e->model.n_plinks, e->model.d_primal, e->stream);   // every message's pairwise slot := its unary's label
    HIP_CHECK(hipGetLastError());
  });
}

int lpmp_compute_pass_custom(lpmp_engine* e, int64_t n, const int32_t* factors, const int64_t* om_off, const double* om,
                             const int64_t* mk_off, const uint8_t* mk) {
  return guarded([&] {
    require_model(e);
    if (n < 0 || (n > 0 && (!factors || !om_off || !mk_off))) throw std::runtime_error("bad argument");
    check_rows(n, om_off, om, mk_off, mk);
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);
    begin_compute(e);
    Schedule s;
    static const double dz = 0; static const uint8_t uz = 0;
    e->model.plan->p.make_schedule(factors, n, om_off, om ? om : &dz, mk_off, mk ? mk : &uz, s);
    check_generic_limits(e->model.plan->p, s);
    // the schedule lives in a scratch buffer of the engine that is refilled in place: no allocation per call
    DevSchedule& d = e->model.scratch;
    upload_schedule(e, s, d, true, e->model.plan->p.force_generic);
    const bool g = e->use_graph; e->use_graph = false;
    try { run_schedule(e, d); } catch (...) { e->use_graph = g; throw; }
    e->use_graph = g;
    HIP_CHECK(hipStreamSynchronize(e->stream));
  });
}

int lpmp_schedule_create(lpmp_engine* e, int64_t n, const int32_t* factors, const int64_t* om_off, const double* om,
                         const int64_t* mk_off, const uint8_t* mk, int* id_out) {
  return lpmp_schedule_create_fused(e, n, factors, om_off, om, mk_off, mk, 0, id_out);
}
int lpmp_schedule_create_fused(lpmp_engine* e, int64_t n, const int32_t* factors, const int64_t* om_off, const double* om,
                               const int64_t* mk_off, const uint8_t* mk, int fuse, int* id_out) {
  return guarded([&] {
    require_model(e);
    if (!id_out || n < 0 || (n > 0 && (!factors || !om_off || !mk_off))) throw std::runtime_error("bad argument");
    check_rows(n, om_off, om, mk_off, mk);
    HIP_CHECK(hipSetDevice(e->device));
    Schedule s;
    static const double dz = 0; static const uint8_t uz = 0;
    static const int64_t zero_off[1] = {0};
    e->model.plan->p.make_schedule(std::vector<Plan::Segment>{Plan::Segment{factors, n, n > 0 ? om_off : zero_off, om ? om : &dz,
                                                                      n > 0 ? mk_off : zero_off, mk ? mk : &uz}},
                             fuse != 0 && e->use_fused, s);
    check_generic_limits(e->model.plan->p, s);
    auto d = std::make_unique<DevSchedule>();
    upload_schedule(e, s, *d, false, e->model.plan->p.force_generic);
    e->model.custom.push_back(std::move(d));
    *id_out = (int)e->model.custom.size() - 1;
  });
}
static DevSchedule& custom_schedule(lpmp_engine* e, int id) {
  require_model(e);
  if (id < 0 || id >= (int)e->model.custom.size() || !e->model.custom[id]) throw std::runtime_error("unknown schedule id");
  return *e->model.custom[id];
}
int lpmp_schedule_run(lpmp_engine* e, int id) {
  return guarded([&] {
    DevSchedule& d = custom_schedule(e, id);
    if (d.adaptive_built != (e->rtype == LPMP_RTYPE_ADAPTIVE))
      throw StateError("this schedule was prepared under another send rule (adaptive sends run on other kernels): create it again");
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);
    begin_compute(e);
    run_schedule(e, d);
  });
}
int lpmp_schedule_info(lpmp_engine* e, int id, int64_t* n_levels, int64_t* n_launches, int64_t* n_recv, int64_t* n_send,
                       int64_t* alg_bytes) {
  return guarded([&] {
    DevSchedule& d = custom_schedule(e, id);
    if (n_levels) *n_levels = d.n_levels;
    if (n_launches) *n_launches = (int64_t)d.launches.size();
    if (n_recv) *n_recv = d.n_recv;
    if (n_send) *n_send = d.n_send;
    if (alg_bytes) *alg_bytes = d.alg_bytes;
  });
}
int lpmp_schedule_destroy(lpmp_engine* e, int id) {
  return guarded([&] {
    (void)custom_schedule(e, id);
    HIP_CHECK(hipStreamSynchronize(e->stream));
    e->model.custom[id].reset();
  });
}

// the chain executor bounds every wait; a run that gave up leaves the duals half updated and must not pass silently
void check_chain(lpmp_engine* e) {
  if (!e->chain_ran || !e->d_chain_abort) return;
  int32_t* h = (int32_t*)(e->pinned + 8 * 1024 + 128);
  static_assert(8 * 1024 + 128 + CHAIN_ABORT_WORDS * 4 <= PINNED_WORDS_BYTES, "pinned block");
  HIP_CHECK(hipMemcpyAsync(h, e->d_chain_abort, CHAIN_ABORT_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
  e->chain_ran = false;
  if (h[0] != 0) {
    std::string what;
    if (h[1] != 0) {
      const long long now = (long long)(((unsigned long long)(unsigned)h[7] << 32) | (unsigned)h[6]), t0 = (long long)(((unsigned long long)(unsigned)h[9] << 32) | (unsigned)h[8]);
      what = h[3] == -2 ? " (a mailbox granule, tag seen " + std::to_string(h[4]) + ", epoch " + std::to_string(h[5])
                        : " (ticket " + std::to_string(h[2]) + " waited for ticket " + std::to_string(h[3]) + ": flag word " + std::to_string(h[4]) + ", epoch " + std::to_string(h[5]);
      what += ", " + std::to_string((double)(now - t0) * 1e-8) + " s, " + std::to_string(h[10]) + " tickets drawn)";
    }
    HIP_CHECK(hipMemsetAsync(e->d_chain_abort, 0, CHAIN_ABORT_WORDS * sizeof(int32_t), e->stream));
    throw DeviceError("chain executor: a dependency wait timed out" + what + "; the duals are in an undefined state (LPMP_NO_CHAIN=1 selects graph replay, LPMP_CHAIN_TIMEOUT_S the bound)");
  }
}

static void compute_factor_lbs(lpmp_engine* e) {
  require_consts(e);
  check_chain(e);
  rows_refresh(e);
  if (e->use_lb_tracking && !e->model.lb_all_stale) {
    // the sweep kernels kept d_lb current except for the entries they marked NaN: recompute only those
    const int64_t nf = e->model.plan->p.nf;
    HIP_CHECK(hipMemsetAsync(e->model.d_stale_n, 0, sizeof(unsigned long long), e->stream));
    launch_lb_collect_stale(e->model.d_lb, nf, e->model.d_stale, e->model.d_stale_n, e->stream);
    HIP_CHECK(hipMemcpyAsync(e->h_stale_n, e->model.d_stale_n, sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIP_CHECK(hipStreamSynchronize(e->stream));
    const int64_t n_stale = (int64_t)*e->h_stale_n;
    if (n_stale <= nf / 8) {
      launch_factor_lb_list(e->model.d_lbrecs, e->model.d_dual, e->model.d_const, e->model.d_lb, e->model.d_stale, n_stale, e->model.tab_flag, e->stream);
      HIP_CHECK(hipGetLastError());
      e->last_lb_recomputed = n_stale;
      return;
    }
  }
  e->last_lb_recomputed = e->model.plan->p.nf;
  for (const auto& r : e->model.lb_runs) {
    if (r.cls == 0 || !launch_dense_lb(r.cls, e->model.d_lbrecs, e->model.d_dual, e->model.d_const, e->model.d_lb, r.first, r.count, e->model.tab_flag, e->stream))
      launch_factor_lb(e->model.d_lbrecs + r.first, e->model.d_dual, e->model.d_const, e->model.d_lb + r.first, r.count, e->model.tab_flag, e->stream);
  }
  HIP_CHECK(hipGetLastError());
  e->model.lb_all_stale = false;
}

int lpmp_lower_bound(lpmp_engine* e, double* out) {
  return guarded([&] {
    require_model(e);
    if (!out) throw std::runtime_error("null argument");
    HIP_CHECK(hipSetDevice(e->device));
    if (spec_lower_bound(e, out)) return;      // the caller is inside a batch of passes that ran ahead: that pass's own row
    compute_factor_lbs(e);
    const int64_t nf = e->model.plan->p.nf;
    int64_t nb = std::min<int64_t>(1024, (nf + 255) / 256);
    const int64_t per = (nf + nb - 1) / nb;
    nb = (nf + per - 1) / per;
    launch_sum_stage(e->model.d_lb, e->model.d_part, nf, per, nb, e->stream);
    HIP_CHECK(hipMemcpyAsync(e->h_part, e->model.d_part, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_CHECK(hipStreamSynchronize(e->stream));
    double lb = e->model.plan->p.constant;
    for (int64_t i = 0; i < nb; ++i) lb += e->h_part[i];
    *out = lb;
  });
}

// the same value into the caller's device memory: no host synchronisation, no device-to-host copy, so the count of stale entries
// stays on the device (the list kernel reads it there) and an aborted chain run is reported by the next call that synchronises.
// lpmp_lower_bound_recomputed keeps the value of the last host call
int lpmp_lower_bound_dev(lpmp_engine* e, double* dst_dev) {
  return guarded([&] {
    require_model(e);
    if (!dst_dev) throw std::runtime_error("lpmp_lower_bound_dev: null destination");
    HIP_CHECK(hipSetDevice(e->device));
    ModelState& m = e->model;
    const int64_t nf = m.plan->p.nf;
    int64_t nb, per; lb_sum_blocks(nf, nb, per);
    const auto& sp = m.batch;
    if (sp.n > 0 && sp.pos >= 1 && sp.pos < sp.n) {   // inside a batch of passes that ran ahead: that pass's own row, as the host call
      launch_sum_final(sp.d_hpart + (size_t)(sp.pos - 1) * 1024, nb, m.plan->p.constant, nullptr, dst_dev, e->stream);
      HIP_CHECK(hipGetLastError());
      return;
    }
    require_consts(e);
    rows_refresh(e);
    if (e->use_lb_tracking && !m.lb_all_stale) {
      HIP_CHECK(hipMemsetAsync(m.d_stale_n, 0, sizeof(unsigned long long), e->stream));
      launch_lb_collect_stale(m.d_lb, nf, m.d_stale, m.d_stale_n, e->stream);
      launch_factor_lb_list_dev(m.d_lbrecs, m.d_dual, m.d_const, m.d_lb, m.d_stale, m.d_stale_n, nf, m.tab_flag, e->stream);
    } else {
      for (const auto& r : m.lb_runs) {
        if (r.cls == 0 || !launch_dense_lb(r.cls, m.d_lbrecs, m.d_dual, m.d_const, m.d_lb, r.first, r.count, m.tab_flag, e->stream))
          launch_factor_lb(m.d_lbrecs + r.first, m.d_dual, m.d_const, m.d_lb + r.first, r.count, m.tab_flag, e->stream);
      }
      m.lb_all_stale = false;
    }
    launch_sum_stage(m.d_lb, m.d_part, nf, per, nb, e->stream);
    launch_sum_final(m.d_part, nb, m.plan->p.constant, nullptr, dst_dev, e->stream);
    HIP_CHECK(hipGetLastError());
  });
}

int lpmp_factor_lower_bounds(lpmp_engine* e, double* out) {
  return guarded([&] {
    require_model(e);
    if (!out) throw std::runtime_error("null argument");
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);
    compute_factor_lbs(e);
    d2h(out, e->model.d_lb, (size_t)e->model.plan->p.nf * sizeof(double), e->stream);
  });
}

int lpmp_synchronize(lpmp_engine* e) {
  return guarded([&] {
    if (!e) throw std::runtime_error("null engine");
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);                                  // after this call the (possibly borrowed) dual buffer holds the caller's state
    rows_flush(e);
    if (e->model.rows && !e->model.own_dual()) e->model.rows_stale = true;   // ... and the caller may write it: the rows are refreshed before the next pass
    HIP_CHECK(hipStreamSynchronize(e->stream));
    if (e->timing) e->drain_timing();
    check_chain(e);
    if (!guarded_ok(e->pinned, PINNED_WORDS_BYTES)) throw DeviceError("guard region of the engine's pinned words was overwritten");
    staging().check();
  });
}

// common entry of the lpmp_boundary_* calls (boundary.hip): the engine's device is current, a speculative batch is
// settled, and an aborted chain run is reported instead of its duals being consumed
int lpmp_boundary_enter(lpmp_engine* e) {
  return guarded([&] {
    if (!e) throw std::runtime_error("null engine");
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);
    check_chain(e);
    // the boundary / halo kernels address dense pairwise vectors through device offsets, i.e. in the ROWS when that layout is on:
    // whatever the caller put into the packed array since the last hand-over (lpmp_upload_duals, a write after lpmp_synchronize /
    // lpmp_device_duals) must be in the rows before they are read, and before lpmp_boundary_leave marks the rows as the newer copy
    rows_refresh(e);
  });
}

int lpmp_streaming_access(const lpmp_engine* e) { return e && e->model.plan ? (e->model.nt_flag ? 1 : 0) : -1; }

int64_t lpmp_dual_size(const lpmp_engine* e) { return e && e->model.plan ? e->model.plan->p.f_doff[e->model.plan->p.nf] : 0; }

int lpmp_download_duals(lpmp_engine* e, double* out) {
  return guarded([&] {
    require_model(e);
    if (!out) throw std::runtime_error("null argument");
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);
    check_chain(e);
    rows_flush(e);
    d2h(out, e->model.d_dual, (size_t)lpmp_dual_size(e) * sizeof(double), e->stream);
  });
}
int lpmp_upload_duals(lpmp_engine* e, const double* in) {
  return guarded([&] {
    require_model(e);
    if (!in) throw std::runtime_error("null argument");
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);
    h2d(e->model.d_dual, in, (size_t)lpmp_dual_size(e) * sizeof(double), e->stream);
    if (e->model.rows) { e->model.rows_stale = true; e->model.packed_stale = false; }
    e->model.lb_all_stale = true;
  });
}
int lpmp_invalidate_lower_bounds(lpmp_engine* e) {
  // (the caller says it wrote the packed dual array behind the engine's back: with the rows layout, what it wrote there for
  // a dense pairwise factor replaces the row's vectors — after what the rows hold has been written out, so that everything
  // the caller did not touch survives)
  return guarded([&] { require_model(e); settle(e); if (e->model.rows) { rows_flush(e); e->model.rows_stale = true; } e->model.lb_all_stale = true; });
}
// ---- new costs on the plan that is already there (include/lpmp_engine.h) --------------------------------------------------------
// all tracked bounds stale, primal labels unset: what every change of costs leaves behind
static void costs_changed(lpmp_engine* e) {
  HIP_CHECK(hipMemsetAsync(e->model.d_lb, 0xFF, (size_t)e->model.plan->p.nf * sizeof(double), e->stream));   // all NaN, as after the upload
  e->model.lb_all_stale = true;
  // (primal_unset_only: labels that a path or forest move wrote into the array of unset labels of a model the rounding code refuses)
  if (e->model.have_primal || e->model.primal_unset_only) { upload_unset_primal(e); e->model.primal_t = 0; }
}
int lpmp_upload_costs(lpmp_engine* e, const double* const_data, int const_mem, const double* dual_data, int dual_mem) {
  return guarded([&] {
    if (!e || !e->model.plan) throw StateError("lpmp_upload_costs: no model uploaded (the structure comes from lpmp_upload_model)");
    if (!const_data && !dual_data) throw StateError("lpmp_upload_costs: neither constants nor duals given");
    HIP_CHECK(hipSetDevice(e->device));
    Plan& p = e->model.plan->p;
    const int64_t n_const = p.f_coff[p.nf], n_dual = p.f_doff[p.nf];
    if (dual_data) {   // cold start: an open batch of passes that ran ahead is dropped, its snapshot is dead
      e->model.batch.n = 0; e->model.batch.pos = 0; e->model.batch.lb_ready = false;
      spec_interrupt(e);
    } else settle(e);  // warm start: the duals are those of the pass the caller is at
    check_chain(e);
    if (dual_data) {
      if (dual_mem != LPMP_MEM_DEVICE) h2d(e->model.d_dual, dual_data, (size_t)n_dual * sizeof(double), e->stream);
      else if (dual_data != e->model.d_dual) HIP_CHECK(hipMemcpyAsync(e->model.d_dual, dual_data, (size_t)n_dual * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      if (e->model.rows) { e->model.rows_stale = true; e->model.packed_stale = false; }
    }
    if (const_data && n_const > 0) {
      const bool dev = const_mem == LPMP_MEM_DEVICE;
      if (!e->model.tab_compact) {   // the packed constants as a whole: the engine's own buffer, or the caller's borrowed one
        if (!dev) h2d(e->model.d_const, const_data, (size_t)n_const * sizeof(double), e->stream);
        else if (const_data != e->model.d_const) HIP_CHECK(hipMemcpyAsync(e->model.d_const, const_data, (size_t)n_const * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      }
      if (e->model.tab_prec != LPMP_TABLES_F64) {
        e->model.const_bad = true;   // until the narrowing has accepted every table
        try { if (e->model.tab_compact) narrow_tables(e->model, e->stream, const_data, dev, false); else narrow_tables(e->model, e->stream, e->model.d_const, true, false); }
        catch (...) { e->model.lb_all_stale = true; throw; }
      }
      e->model.const_bad = false;
      gather_shared_cells(e->model, e->stream);
      if (e->model.rows) {
        // the rows take their tables from the constants and their vectors from the packed duals: the packed array first gets what
        // the rows hold that it does not (warm start), then every row is built as at the upload
        if (e->model.rows_stale && e->model.packed_stale) throw StateError("rows layout: packed duals and rows both hold newer vectors");
        rows_flush(e);
        build_rows(e->model, e->stream);
        e->model.rows_stale = false;
      }
    }
    costs_changed(e);
    HIP_CHECK(hipStreamSynchronize(e->stream));   // the caller's arrays are the caller's again
  });
}

int lpmp_set_vectors(lpmp_engine* e, int64_t n, const int32_t* factors, const double* src, int64_t src_stride, int src_mem, int accumulate) {
  return guarded([&] {
    require_model(e);
    if (n < 0 || (n > 0 && (!factors || !src))) throw std::runtime_error("lpmp_set_vectors: bad argument");
    HIP_CHECK(hipSetDevice(e->device));
    const Plan& p = e->model.plan->p;
    // (vector factors live in the packed array under every layout)
    const ListedSrc s = listed_rows(e, "lpmp_set_vectors", n, factors, src, src_stride, src_mem == LPMP_MEM_DEVICE, true, " is not a VECTOR factor", e->model.d_setrecs,
                                    [&](int64_t, int32_t f, int64_t src_row) { return SetVecRec{p.f_doff[f], src_row, p.f_dim0[f], f}; });
    if (n == 0) return;
    launch_set_vectors(e->model.d_setrecs, n, s.src, s.stride, e->model.d_dual, e->model.d_lb, accumulate != 0, e->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(e->stream));   // the record buffer is refilled by the next call; the caller's source is the caller's again
  });
}

int lpmp_upload_shared_pool(lpmp_engine* e, const double* sh_data, int sh_mem) {
  return guarded([&] {
    if (!e || !e->model.plan) throw StateError("lpmp_upload_shared_pool: no model uploaded (the structure comes from lpmp_upload_model)");
    if (!sh_data) throw std::runtime_error("lpmp_upload_shared_pool: null argument");
    Plan& p = e->model.plan->p;
    if (p.n_shared <= 0 || !e->model.d_shared) throw std::runtime_error("lpmp_upload_shared_pool: the model has no pool of shared tables");
    HIP_CHECK(hipSetDevice(e->device));
    // the band detection and the NaN refusal read the values on the host: a device source (KBs to a few MB) is copied there first
    std::vector<double> host;
    if (sh_mem == LPMP_MEM_DEVICE) {
      host.resize((size_t)p.sh_off[(size_t)p.n_shared]);
      d2h(host.data(), sh_data, host.size() * sizeof(double), e->stream);
      sh_data = host.data();
    }
    settle(e);          // the duals are those of the pass the caller is at (as the warm start of lpmp_upload_costs)
    check_chain(e);
    e->model.plan->set_shared_pool(sh_data);          // (a NaN entry: thrown before anything has changed)
    HIP_CHECK(hipStreamSynchronize(e->stream));   // no launch in flight reads the pool while it is rewritten
    write_shared_pool(e->model, e->stream, (int64_t)e->model.sh_cells.size() / 2);
    e->model.for_each_schedule([&](DevSchedule& d) { d.refresh_diff_band(p); });
    costs_changed(e);
    HIP_CHECK(hipStreamSynchronize(e->stream));
  });
}

int lpmp_set_constants(lpmp_engine* e, int64_t n, const int32_t* factors, const double* src, int64_t src_stride, int src_mem) {
  return guarded([&] {
    require_model(e);
    if (n < 0 || (n > 0 && (!factors || !src))) throw std::runtime_error("lpmp_set_constants: bad argument");
    HIP_CHECK(hipSetDevice(e->device));
    ModelState& m = e->model;
    const Plan& p = m.plan->p;
    const bool f32 = m.tab_prec != LPMP_TABLES_F64;
    const int64_t sh_base = m.d_shared ? (int64_t)(((intptr_t)m.d_shared.get() - (intptr_t)m.d_const) / 8) : 0;
    bool any_f32 = false;
    const ListedSrc s = listed_rows(e, "lpmp_set_constants", n, factors, src, src_stride, src_mem == LPMP_MEM_DEVICE, false,
                                    " is a VECTOR factor (its costs are duals: lpmp_set_vectors)", m.d_setcrecs, [&](int64_t, int32_t f, int64_t src_row) {
      SetConstRec r{p.coff(f), 0, src_row, (int32_t)(p.f_coff[f + 1] - p.f_coff[f]), f, 0, 0};
      if (p.f_kind[f] == LPMP_F_PAIRWISE_DENSE) {
        if (f32) { r.f32 = 1; any_f32 = true; }                       // the float table only: nothing is written as doubles
        else if (m.rows) { r.dst = p.f_coff[f]; r.dst2 = p.coff(f); r.two = 1; }   // the packed table, and the table part of the factor's row
      } else if (p.f_kind[f] == LPMP_F_PAIRWISE_SHARED || p.f_kind[f] == LPMP_F_PAIRWISE_DIFF || p.f_kind[f] == LPMP_F_PAIRWISE_DIFF_SHIFT) {
        // the first word of the factor's cell, and the scalar lpmp_upload_costs would gather the cell from again (DIFF_SHIFT, two: the
        // first words of its two cells — every second word from r.dst on — and the two scalars)
        const bool shift = p.f_kind[f] == LPMP_F_PAIRWISE_DIFF_SHIFT;
        const int64_t k = (r.dst - sh_base) / 2;
        if (k < 0 || 2 * k + (shift ? 3 : 1) >= (int64_t)m.sh_cells.size() || sh_base + 2 * k != r.dst) throw std::runtime_error("lpmp_set_constants: internal: factor " + std::to_string(f) + " has no cell");
        r.dst2 = m.sh_cells[(size_t)(2 * k)]; r.two = shift ? 2 : 1;
      }
      return r;
    });
    if (n == 0) return;
    if (any_f32) {
      // a listed set is small: every row of a float table is checked BEFORE anything is written, so a refusal leaves the old costs
      // whole (stronger than lpmp_upload_costs, which cannot afford a pass over all tables)
      const int strict = m.tab_prec == LPMP_TABLES_F32 ? 1 : 0;
      DevBuf<int> d_bad; d_bad.alloc(1);
      int bad = INT32_MAX;
      h2d(d_bad, &bad, sizeof(int), e->stream);
      launch_set_constants_check(m.d_setcrecs, n, s.src, s.stride, strict, d_bad, e->stream);
      HIP_CHECK(hipGetLastError());
      d2h(&bad, d_bad, sizeof(int), e->stream);
      HIP_CHECK(hipStreamSynchronize(e->stream));
      if (bad != INT32_MAX) throw UnsupportedError(f32_refusal("lpmp_set_constants: ", strict != 0, "row", bad, "; nothing was written"));
    }
    launch_set_constants(m.d_setcrecs, n, s.src, s.stride, m.d_const, m.d_lb, e->stream);
    HIP_CHECK(hipGetLastError());
    if (m.have_primal || m.primal_unset_only) { upload_unset_primal(e); m.primal_t = 0; }   // as after lpmp_upload_costs: the labels belong to the old costs
    HIP_CHECK(hipStreamSynchronize(e->stream));   // the record buffer is refilled by the next call; the caller's source is the caller's again
  });
}

int lpmp_zero_pairwise_duals(lpmp_engine* e) {
  return guarded([&] {
    require_model(e);
    HIP_CHECK(hipSetDevice(e->device));
    settle(e);
    check_chain(e);
    const Plan& p = e->model.plan->p;
    if (e->model.n_zero < 0) {   // once per model: the pairwise factors' vectors where the kernels address them, contiguous runs merged, cut into pieces
      std::vector<ZeroRec> runs, recs;
      for (int64_t f = 0; f < p.nf; ++f) {
        if (p.f_kind[f] == LPMP_F_VECTOR) continue;
        const int64_t off = p.doff(f), len = (int64_t)p.f_dim0[f] + p.f_dim1[f];
        if (!runs.empty() && runs.back().dual_off + runs.back().len == off) runs.back().len += len; else runs.push_back({off, len});
      }
      for (const ZeroRec& r : runs)
        for (int64_t a = 0; a < r.len; a += ZERO_RUN_MAX) recs.push_back({r.dual_off + a, std::min(ZERO_RUN_MAX, r.len - a)});
      if (!recs.empty()) { e->model.d_zero.alloc(recs.size()); h2d(e->model.d_zero, recs.data(), recs.size() * sizeof(ZeroRec), e->stream); }
      e->model.n_zero = (int64_t)recs.size();
    }
    // (dense pairwise vectors live in the rows under the rows layout: what the caller put into the packed array goes there first, and
    // from here on the rows are the newer copy — as for a pass)
    rows_refresh(e);
    if (e->model.rows) e->model.packed_stale = true;
    launch_zero_pairwise(e->model.d_zero, e->model.n_zero, e->model.d_dual, e->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemsetAsync(e->model.d_lb, 0xFF, (size_t)p.nf * sizeof(double), e->stream));
    e->model.lb_all_stale = true;
  });
}

int64_t lpmp_schedules_built(const lpmp_engine* e) { return e && e->model.plan ? e->model.schedules_built : 0; }

// The packed dual array (serialize_dual order) on the device.  With the rows layout the dense pairwise factors' vectors are
// written out to it first (stream-ordered on the engine's stream), and the caller is assumed to write it: the rows are
// refreshed from it before the next pass — callers that only read may say so by not calling this between passes.
void* lpmp_device_duals(lpmp_engine* e) {
  if (!e) return nullptr;
  if (e->model.rows) { try { (void)hipSetDevice(e->device); rows_flush(e); e->model.rows_stale = true; } catch (const std::exception& ex) { g_error = ex.what(); return nullptr; } }
  return e->model.d_dual;
}
// internal (boundary.hip): the base pointer itself, and where a packed dual offset lives on the device
void* lpmp_engine_dual_base(lpmp_engine* e) { return e ? e->model.d_dual : nullptr; }
int64_t lpmp_engine_device_dual_offset(lpmp_engine* e, int64_t packed_off) {
  if (!e || !e->model.plan || e->model.plan->p.dev_doff.empty()) return packed_off;
  const Plan& p = e->model.plan->p;
  const int64_t f = (int64_t)(std::upper_bound(p.f_doff.begin(), p.f_doff.end(), packed_off) - p.f_doff.begin()) - 1;
  if (f < 0 || f >= p.nf) return packed_off;
  return p.dev_doff[f] + (packed_off - p.f_doff[f]);
}
// internal (boundary.hip): is [packed_off, packed_off + len) a run of doubles inside ONE factor's dual?  (what the device
// offset mapping above and the kernels that follow it assume)
int lpmp_engine_dual_range_ok(lpmp_engine* e, int64_t packed_off, int64_t len) {
  if (!e || !e->model.plan || len < 0 || packed_off < 0) return 0;
  const Plan& p = e->model.plan->p;
  if (packed_off + len > p.f_doff[p.nf]) return 0;
  if (len == 0) return 1;
  const int64_t f = (int64_t)(std::upper_bound(p.f_doff.begin(), p.f_doff.end(), packed_off) - p.f_doff.begin()) - 1;
  return f >= 0 && f < p.nf && packed_off + len <= p.f_doff[f + 1] ? 1 : 0;
}
int lpmp_boundary_leave(lpmp_engine* e) {      // a boundary kernel wrote duals through device offsets: only the tracked bounds are stale
  return guarded([&] { require_model(e); e->model.lb_all_stale = true; if (e->model.rows) e->model.packed_stale = true; });
}
// Persistent launches (chain executor, joined passes in Infinity-Cache order) assume that resident workgroups keep running, i.e.
// that the device is this process's own (kernels.hip): a host that knows it shares the device switches them off per engine.
// The environment's LPMP_NO_CHAIN / LPMP_NO_BLOCKED_PASSES keep the last word (off stays off).
int lpmp_set_persistent_launches(lpmp_engine* e, int on) {
  return guarded([&] {
    if (!e) throw std::runtime_error("null engine");
    if (e->model.plan) { HIP_CHECK(hipSetDevice(e->device)); settle(e); }
    const char* nc = std::getenv("LPMP_NO_CHAIN"); const char* nb = std::getenv("LPMP_NO_BLOCKED_PASSES");
    e->use_chain = on != 0 && !(nc && nc[0] == '1');
    e->use_blocked_passes = on != 0 && !(nb && nb[0] == '1');
  });
}
int lpmp_persistent_launches(const lpmp_engine* e) { return e && e->use_chain && e->use_blocked_passes ? 1 : 0; }
// "pci=<domain:bus:device.function> uuid=<32 hex digits>" of a HIP device ordinal: what tells two ranks that they sit on the same
// physical GPU when every rank has a visibility mask of its own (then both see "device 0")
int lpmp_device_identity(int device, char* out, int64_t cap) {
  return guarded([&] {
    if (!out || cap < 64) throw std::runtime_error("lpmp_device_identity: buffer of at least 64 bytes needed");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw DeviceError("no HIP device available");
    if (device < 0 || device >= n) throw DeviceError("device ordinal out of range");
    char pci[32] = {0};
    HIP_CHECK(hipDeviceGetPCIBusId(pci, (int)sizeof(pci), device));
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    std::string s = std::string("pci=") + pci + " uuid=";
    static const char* hex = "0123456789abcdef";
    for (unsigned char c : prop.uuid.bytes) { s += hex[c >> 4]; s += hex[c & 15]; }
    if ((int64_t)s.size() + 1 > cap) s.resize((size_t)cap - 1);
    std::memcpy(out, s.c_str(), s.size() + 1);
  });
}
int lpmp_set_rows_layout(lpmp_engine* e, int on) {
  return guarded([&] { if (!e) throw std::runtime_error("null engine"); e->want_rows = on != 0; });
}
int lpmp_rows_layout(const lpmp_engine* e) { return e && e->model.rows ? 1 : 0; }
int lpmp_set_table_precision(lpmp_engine* e, int precision) {
  return guarded([&] {
    if (!e) throw std::runtime_error("null argument");
    if (precision != LPMP_TABLES_F64 && precision != LPMP_TABLES_F32 && precision != LPMP_TABLES_F32_ROUND) throw std::runtime_error("unknown table precision");
    e->want_tab = precision;
  });
}
int lpmp_table_precision(const lpmp_engine* e) { return e ? e->model.tab_prec : LPMP_TABLES_F64; }
int lpmp_plan_set_table_precision(lpmp_plan* p, int precision) {
  return guarded([&] {
    if (!p) throw std::runtime_error("null argument");
    if (precision != LPMP_TABLES_F64 && precision != LPMP_TABLES_F32 && precision != LPMP_TABLES_F32_ROUND) throw std::runtime_error("unknown table precision");
    const bool f32 = precision != LPMP_TABLES_F64;
    if (f32 != p->p.tables_f32) { p->p.tables_f32 = f32; p->drop_caches(); }
  });
}
int64_t lpmp_lower_bound_recomputed(const lpmp_engine* e) { return e ? e->last_lb_recomputed : -1; }
void* lpmp_engine_stream(lpmp_engine* e) { return e ? (void*)e->stream : nullptr; }
const lpmp_plan* lpmp_engine_plan(const lpmp_engine* e) { return e ? e->model.plan.get() : nullptr; }
lpmp_plan* lpmp_engine_plan_mut(lpmp_engine* e) { return e ? e->model.plan.get() : nullptr; }

int lpmp_enable_kernel_timing(lpmp_engine* e, int on) {
  return guarded([&] {
    if (!e) throw std::runtime_error("null engine");
    settle(e);
    HIP_CHECK(hipStreamSynchronize(e->stream));
    if (e->timing) e->drain_timing();
    e->timing = on != 0;
  });
}
int lpmp_get_kernel_timing(lpmp_engine* e, int n, double* ms, int64_t* launches, int64_t* factors, int64_t* receives, int64_t* bytes) {
  return guarded([&] {
    if (!e) throw std::runtime_error("null engine");
    HIP_CHECK(hipStreamSynchronize(e->stream));
    e->drain_timing();
    for (int c = 0; c < n && c < KC_COUNT; ++c) {
      if (ms) ms[c] = e->ct[c].ms;
      if (launches) launches[c] = e->ct[c].launches;
      if (factors) factors[c] = e->ct[c].factors;
      if (receives) receives[c] = e->ct[c].receives;
      if (bytes) bytes[c] = e->ct[c].bytes;
    }
  });
}
// of the launches lpmp_get_kernel_timing reports per class: how many were persistent chain-executor launches
int lpmp_get_chain_launches(lpmp_engine* e, int n, int64_t* chain_launches) {
  return guarded([&] {
    if (!e || !chain_launches) throw std::runtime_error("null argument");
    HIP_CHECK(hipStreamSynchronize(e->stream));
    e->drain_timing();
    for (int c = 0; c < n && c < KC_COUNT; ++c) chain_launches[c] = e->ct[c].chain_launches;
  });
}
// joined-pass launches in the peer-minima form (W publishes, K / T read no table) since the last lpmp_reset_kernel_timing; counted
// whether or not timing is on — with timing on from the reset, it is a part of the class's chain launches
int lpmp_get_peer_minima_launches(lpmp_engine* e, int64_t* launches) {
  return guarded([&] {
    if (!e || !launches) throw std::runtime_error("null argument");
    HIP_CHECK(hipStreamSynchronize(e->stream));
    e->drain_timing();
    *launches = e->ct[KC_DENSE_32].peer_minima_launches;
  });
}
// of the launches lpmp_get_kernel_timing reports for class diff: how many ran sweep_diff_band_kernel
int lpmp_get_diff_band_launches(lpmp_engine* e, int64_t* band_launches) {
  return guarded([&] {
    if (!e || !band_launches) throw std::runtime_error("null argument");
    HIP_CHECK(hipStreamSynchronize(e->stream));
    e->drain_timing();
    *band_launches = e->ct[KC_DIFF].band_launches;
  });
}
// ... and how many had a DIFF_SHIFT factor (sweep_diff_shift_kernel or sweep_diff_shift_band_kernel)
int lpmp_get_diff_shift_launches(lpmp_engine* e, int64_t* shift_launches) {
  return guarded([&] {
    if (!e || !shift_launches) throw std::runtime_error("null argument");
    HIP_CHECK(hipStreamSynchronize(e->stream));
    e->drain_timing();
    *shift_launches = e->ct[KC_DIFF].shift_launches;
  });
}
// ... and of those, how many ran sweep_diff_shift_band_kernel
int lpmp_get_diff_shift_band_launches(lpmp_engine* e, int64_t* shift_band_launches) {
  return guarded([&] {
    if (!e || !shift_band_launches) throw std::runtime_error("null argument");
    HIP_CHECK(hipStreamSynchronize(e->stream));
    e->drain_timing();
    *shift_band_launches = e->ct[KC_DIFF].shift_band_launches;
  });
}
int lpmp_reset_kernel_timing(lpmp_engine* e) {
  return guarded([&] {
    if (!e) throw std::runtime_error("null engine");
    HIP_CHECK(hipStreamSynchronize(e->stream));
    e->drain_timing();
    for (auto& c : e->ct) c = ClassTiming();
  });
}

int lpmp_synth_fill(void* p, int64_t n, uint64_t seed, uint64_t first, void* stream) {
  return guarded([&] {
    if (!p && n > 0) throw std::runtime_error("null argument");
    launch_synth_fill((double*)p, n, seed, first, (hipStream_t)stream);
    HIP_CHECK(hipGetLastError());
  });
}
