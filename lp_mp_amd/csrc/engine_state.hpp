// engine_state.hpp — what the host translation units of the engine (engine.cpp, prepared.cpp) share: the error types and guarded,
// DevBuf and the staged copies, the uploaded model (ModelState) and the engine, and the entry steps every call goes through.
// C++ only and internal: not part of the ABI (include/lpmp_engine.h), not seen by the kernels or the planner.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "kernels.hpp"

namespace lpmp {
namespace host {

struct DeviceError : std::runtime_error { using std::runtime_error::runtime_error; };
struct StateError : std::runtime_error { using std::runtime_error::runtime_error; };
struct UnsupportedError : std::runtime_error { using std::runtime_error::runtime_error; };

#define HIP_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw DeviceError(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

template <class F>
int guarded(F&& f) {
  try { f(); return LPMP_OK; }
  catch (const DeviceError& e) { lpmp_set_last_error(e.what()); return LPMP_ERR_DEVICE; }
  catch (const StateError& e) { lpmp_set_last_error(e.what()); return LPMP_ERR_STATE; }
  catch (const UnsupportedError& e) { lpmp_set_last_error(e.what()); return LPMP_ERR_UNSUPPORTED; }
  catch (const lpmp::UnsupportedModel& e) { lpmp_set_last_error(e.what()); return LPMP_ERR_UNSUPPORTED; }   // (the planner's size limits)
  catch (const std::bad_alloc&) { lpmp_set_last_error("out of host memory"); return LPMP_ERR_INVALID; }
  catch (const std::exception& e) { lpmp_set_last_error(e.what()); return LPMP_ERR_INVALID; }
}

// A device allocation that frees itself: move-only, empty or `capacity()` elements.  The only place of the host code that calls
// hipMalloc / hipFree.  Freeing (reset, destructor, move assignment) never throws; hipFree waits for the device.
template <class T>
class DevBuf {
  T* p_ = nullptr; size_t cap_ = 0;
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; } return *this; }
  ~DevBuf() { reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t capacity() const { return cap_; }
  void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; cap_ = 0; }
  // a fresh allocation of n elements (what the buffer held is freed first); try_alloc reports a failure instead of throwing
  bool try_alloc(size_t n) {
    reset();
    if (hipMalloc((void**)&p_, n * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); p_ = nullptr; return false; }
    cap_ = n;
    return true;
  }
  void alloc(size_t n) { reset(); HIP_CHECK(hipMalloc((void**)&p_, n * sizeof(T))); cap_ = n; }
  // a buffer that is refilled in place: a new allocation only when n exceeds the capacity, then with a quarter to spare
  void grow(size_t n) { if (n > cap_) alloc(n + n / 4 + 16); }
};
struct GraphExec {   // an instantiated graph, destroyed with its owner; move-only
  hipGraphExec_t g = nullptr;
  GraphExec() = default;
  GraphExec(const GraphExec&) = delete;
  GraphExec& operator=(const GraphExec&) = delete;
  GraphExec(GraphExec&& o) noexcept : g(o.g) { o.g = nullptr; }
  GraphExec& operator=(GraphExec&& o) noexcept { if (this != &o) { reset(); g = o.g; o.g = nullptr; } return *this; }
  ~GraphExec() { reset(); }
  void reset() { if (g) { (void)hipGraphExecDestroy(g); g = nullptr; } }
};

// chain executor (deep schedules): the device copy of a ChainPlan, or of the ticket lists of n joined passes
struct DevChain {
  int32_t kclass = 0, tickets = 0, epoch = 0;
  bool banded = false;                     // Infinity-Cache ticket order: plain table loads, not the streaming policy
  bool level_loop = false;                 // one workgroup walks the launches (tiny levels of a generic class)
  // entries of `launches`: what the level loop walks, and, set for every chain of joined passes (rotation_chain), what the kernel with
  // tickets ahead copies to LDS (at most PQ_AHEAD_MAX_LAUNCHES)
  int32_t n_launches = 0;
  DevBuf<ChainLaunch> launches; DevBuf<int32_t> tk_launch, tk_block, dep_off, dep, done, next;
  DevBuf<int32_t> desc; int32_t desc_inline = 0;   // one descriptor per ticket (plan.hpp ticket_descriptors): the joined passes whose kernel takes tickets ahead
  DevBuf<unsigned long long> mailbox;      // tagged granules of the message vectors that travel between dependent records (chain_plan.cpp)
};
// what issue_launches reads of a schedule: its device arrays and a list of its launches
struct LaunchView { const UpdRec* recs; const Op* ops; const Op* packets; const std::vector<LevelRange>& launches; };

struct DevSchedule {
  DevBuf<UpdRec> recs; DevBuf<Op> ops, packets;   // (a scratch schedule is refilled in place: DevBuf::grow)
  std::vector<LevelRange> launches;
  std::vector<int32_t> diff_tab_off, diff_tab, diff_tab_ne;   // Schedule::diff_tab_off / diff_tab / diff_tab_ne: what new pool values ask again (refresh_diff_band)
  int64_t n_levels = 0, n_recv = 0, n_send = 0, alg_bytes = 0;
  GraphExec graph, graph_primal;           // graph_primal: the same launches with the SWEEP_PRIMAL flag
  bool adaptive_built = false;             // built with every update on the generic kernels (adaptive send rule)
  std::vector<DevChain> chains;            // one per kernel class; the other launches stay plain
  std::vector<LevelRange> plain;           // launches that do not belong to a chain
  bool chain = false;
  LaunchView view() const { return {recs, ops, packets, launches}; }
  LaunchView plain_view() const { return {recs, ops, packets, plain}; }
  void release_chain() { chains.clear(); plain.clear(); chain = false; }
  void release() {
    graph.reset(); graph_primal.reset();
    recs.reset(); ops.reset(); packets.reset();
    release_chain();
    launches.clear(); diff_tab_off.clear(); diff_tab.clear(); diff_tab_ne.clear();
  }
  // new pool values: diff_band / diff_shift_band of the KC_DIFF launches again; a graph captured with the other kernel choice is never replayed
  void refresh_diff_band(const Plan& p) {
    const bool a = p.refresh_diff_band(launches, diff_tab_off, diff_tab, diff_tab_ne), b = p.refresh_diff_band(plain, diff_tab_off, diff_tab, diff_tab_ne);
    bool diff = false;
    for (const auto& lr : launches) diff = diff || lr.kclass == KC_DIFF;
    if (a || b || diff) { graph.reset(); graph_primal.reset(); }
  }
};

struct ClassTiming { double ms = 0; int64_t launches = 0, factors = 0, receives = 0, bytes = 0, chain_launches = 0, band_launches = 0, shift_launches = 0, shift_band_launches = 0, peer_minima_launches = 0; };

}  // namespace host
}  // namespace lpmp
using namespace lpmp;
using namespace lpmp::host;

struct lpmp_plan {
  Plan p;
  RotationInfo rot[LPMP_REPAM_COUNT];
  Schedule sched_cache[2][LPMP_REPAM_COUNT]; bool have_sched[2][LPMP_REPAM_COUNT] = {{false}};
  Schedule pass_cache[LPMP_REPAM_COUNT]; bool have_pass[LPMP_REPAM_COUNT] = {false};   // forward+backward as one fused sequence
  Schedule bf_cache[LPMP_REPAM_COUNT]; bool have_bf[LPMP_REPAM_COUNT] = {false};       // backward+forward (the seam between two passes)
  bool rotation_ok[LPMP_REPAM_COUNT] = {false};
  DecodePlan decode_cache[2]; bool have_decode[2] = {false, false};   // conditional rounding (structure only: no weights, no mode)
  const DecodePlan& decode(int d) {
    if (!have_decode[d]) { decode_cache[d] = p.decode_plan(d); have_decode[d] = true; }
    return decode_cache[d];
  }
  // new VALUES for the pool (Plan::set_shared_pool): of the cached schedules only diff_band / diff_shift_band of their KC_DIFF launches move
  void set_shared_pool(const double* values) {
    p.set_shared_pool(values);
    auto again = [&](Schedule& s) { p.refresh_diff_band(s.launches, s.diff_tab_off, s.diff_tab, s.diff_tab_ne); };
    for (int m = 0; m < LPMP_REPAM_COUNT; ++m) {
      for (int d = 0; d < 2; ++d) again(sched_cache[d][m]);
      again(pass_cache[m]); again(bf_cache[m]);
    }
  }
  void drop_caches() {   // the kernel classes of every schedule change with Plan::force_generic
    for (int m = 0; m < LPMP_REPAM_COUNT; ++m) {
      for (int d = 0; d < 2; ++d) { sched_cache[d][m] = Schedule(); have_sched[d][m] = false; }
      pass_cache[m] = Schedule(); have_pass[m] = false; bf_cache[m] = Schedule(); have_bf[m] = false; rotation_ok[m] = false;
    }
  }
};

// the uploaded model and its parts: internal to the engine's host code
namespace lpmp {
namespace host {

// joined passes as one persistent launch: expansions of RotationInfo, by mode and pass count
struct RotChain {
  DevChain dc; int n_steps = 0; int64_t factors = 0, recv = 0, bytes = 0; uint64_t last_use = 0; size_t dev_bytes = 0;
  // periodic form (rotation_chain): dc holds the TEMPLATE of n_tmpl passes whose tickets [per_begin, per_begin + per_len) are
  // one group of `depth` steps that an n-pass launch executes 1 + (n - n_tmpl) / (depth / 2) times; per_* sums: one period
  bool periodic = false; int n_tmpl = 0, depth = 0; int32_t per_begin = 0, per_len = 0, ring = 0;
  bool peer_minima = false;       // the steps carry CHAIN_LAUNCH_PQ_* roles: launched with the engine's peerq buffer
  bool pq_wide = false;           // ... and the H / K / T blocks hold PQ_WIDE_RECORDS records (ModelState::rot_wide): the wide consume form
  int pq_ahead = 0;               // ... and dc carries ticket descriptors: launched as chain_dense_pq_ahead_kernel (the engine's pq_ahead value)
  int64_t per_factors = 0, per_recv = 0, per_bytes = 0;
};
// the order of a mode's joined passes (order.cpp): its window, computed once, and its tiles, grown the first time a call wants them
// (tile_sets: one per tile size asked for — short and long calls of one model may take different sizes, and both stay)
struct RotOrder { bool have_geo = false; RotGeometry geo; std::map<int, TileSet> tile_sets; bool have_pq_geo = false; PqGeometry pq_geo; };
// conditional rounding from the duals (lpmp_decode_primal): per direction the records sorted by (level, lane-group / wave class),
// their links, and one launch per level and class.  Structure only: built on first use, kept until the next lpmp_upload_model
struct DevDecode {
  struct Launch { int64_t first, count; int32_t width, level; };
  bool have = false;
  DevBuf<DecodeRec> recs; DevBuf<DecodeLink> links;
  std::vector<Launch> launches;
  void release() { have = false; recs.reset(); links.reset(); launches.clear(); }
};
struct LbRun { int cls; int64_t first, count; };
// speculative passes: the open batch and what the engine has learnt of the caller on this model; a fresh value
// is "no batch, nothing learnt, no buffers"
struct SpecBatch {
  int n = 0, pos = 0, mode = -1;     // the open batch: n passes were launched as one chain, the caller has asked for pos of them
  int run_len = 0, learned = 0, last_batch = 0;   // plain single passes since the last other call; length of the previous such run
  bool lb_ready = false; std::vector<double> lb;   // bounds after passes 1 ... n - 1 of the batch
  DevBuf<double> d_snap;             // duals (+ tracked bounds) at the start of the batch
  DevBuf<double> d_hist;             // (n - 1) rows of per-factor bounds
  DevBuf<double> d_hpart;            // partial sums of those rows
  bool snap_lb_stale = false;
};

// Everything that belongs to the uploaded model.  A default-constructed value is "no model" (plan empty); lpmp_upload_model builds
// one as a local and commits it by move, so a refused upload leaves nothing behind, and a member added here needs no line anywhere
// else to be dropped with its model.
struct ModelState {
  std::unique_ptr<lpmp_plan> plan;
  // the base pointers the kernels use, and beside each the engine's own allocation: empty when the caller's memory is borrowed (LPMP_MEM_DEVICE)
  double* d_dual = nullptr; DevBuf<double> dual_buf; bool own_dual() const { return dual_buf.get() != nullptr; }
  double* d_const = nullptr; DevBuf<double> const_buf;
  DevBuf<int32_t> d_tabs;
  DevBuf<LbRec> d_lbrecs;
  DevBuf<double> d_lb, d_part;
  // tracked per-factor lower bounds (kernels.hip): d_lb[f] is valid or NaN; lb_all_stale: recompute everything
  DevBuf<int32_t> d_stale; DevBuf<unsigned long long> d_stale_n;
  bool lb_all_stale = true;
  // primal rounding: the factors' primal_ members, the lazily initialised set, the message links
  DevBuf<int32_t> d_primal;
  DevBuf<PrimalInit> d_pinit; int64_t n_pinit = 0;
  DevBuf<PrimalLink> d_plinks; int64_t n_plinks = 0, n_pprop = 0;   // all messages; the first n_pprop propagate labels
  DevBuf<int32_t> d_pw_unary;     // [2 nf] the unary on each side of a pairwise factor; only with pairwise types that round themselves
  DevBuf<double> d_pcost; DevBuf<int> d_pbad;
  uint64_t primal_t = 0;          // primal_access_ of every factor a primal pass touches (they move together)
  bool have_primal = false;
  bool primal_unset_only = false; // d_primal holds only the unset labels of a model the rounding code refuses (lpmp_readout_labels)
  DevDecode decode[2];
  // rows layout (kernels.hip, rows_copy_kernel): dense pairwise factors live as [table | m1 | m2] rows of d_rows; the packed
  // dual array keeps the vector factors and is the format of every call that hands duals over.  packed_stale: the rows hold
  // newer message vectors than the packed array; rows_stale: the packed array was (or may have been) written by the caller
  bool rows = false, packed_stale = false, rows_stale = false;
  DevBuf<double> d_rows; DevBuf<RowRec> d_rowrecs; int64_t n_rowrecs = 0;
  // shared pairwise tables: [two words {scale, table offset} per SHARED factor | the pool], an allocation of the engine's own
  // that the SHARED factors' device const offsets point into (Plan::dev_coff), and the pool's tables as the shared classes' kernel sees them
  DevBuf<double> d_shared; DevBuf<ShTableDesc> d_sh_desc;
  int nt_flag = 0;                // SWEEP_NT when tables + duals are far larger than L2 + Infinity Cache
  // table precision (lpmp_set_table_precision): the engine's want_tab applies to the next upload, tab_prec is the uploaded model's; with
  // an f32 mode the dense tables live as floats in d_tab32 (every table 16-byte aligned), the DENSE factors' device const offsets point
  // there (Plan::dev_coff, still in 8-byte units relative to d_const) and every launch carries tab_flag = SWEEP_TAB32
  int tab_prec = LPMP_TABLES_F64, tab_flag = 0;
  DevBuf<float> d_tab32;
  bool model_big = false;         // tables + duals > 1 GiB: only then is an Infinity-Cache ticket order worth a chain launch
  // new costs on the planned model (lpmp_upload_costs, lpmp_set_vectors, lpmp_zero_pairwise_duals): everything below is a function
  // of the structure, kept so that the engine-private copies of the constants can be derived again without planning anything
  int64_t schedules_built = 0;    // schedules, chain plans and joined-pass templates planned and uploaded for this model
  bool const_bad = false;         // a refused lpmp_upload_costs left the constants unspecified: nothing may read them
  bool tab_compact = false;       // f32 tables from host memory: const_buf holds only the cells of the non-DENSE factors
  std::vector<int64_t> sh_cells;  // the SHARED / DIFF cells as launch_shared_cells receives them: {const offset, table offset}; a DIFF_SHIFT factor has two in a row, the second {const offset of its shift, length of D}
  DevBuf<SetVecRec> d_setrecs; DevBuf<double> d_setsrc;   // records and (host sources) rows of lpmp_set_vectors, refilled in place
  DevBuf<SetConstRec> d_setcrecs;                         // records of lpmp_set_constants (its host rows share d_setsrc)
  DevBuf<ZeroRec> d_zero; int64_t n_zero = -1;            // pieces of the pairwise message vectors; -1: not built yet
  // prepared read-outs (lpmp_readout_*): model_gen names the uploaded model (unique over all engines of the process; a read-out
  // remembers the one it was made for), d_readout is where a call with a HOST destination lets the kernel write before the copy
  uint64_t model_gen = 0;
  DevBuf<double> d_readout;
  std::vector<LbRun> lb_runs;
  DevSchedule sched[2][LPMP_REPAM_COUNT];
  bool have_sched[LPMP_REPAM_COUNT] = {false, false, false, false};
  DevSchedule sched_pass[LPMP_REPAM_COUNT];            // fused forward+backward (ComputePass)
  DevSchedule sched_bf[LPMP_REPAM_COUNT];              // fused backward+forward: its middle step joins two passes
  DevSchedule sched_part[2]; bool have_part[2] = {false, false};   // compute_partition_pass / compute_overlapping_partition_pass as ONE sequence
  bool rotation_ok[LPMP_REPAM_COUNT] = {false, false, false, false};
  bool have_pass[LPMP_REPAM_COUNT] = {false, false, false, false};
  bool pass_chain_tried[LPMP_REPAM_COUNT] = {};   // ensure_pass_chain_plan ran for that mode
  std::vector<std::unique_ptr<DevSchedule>> custom;   // prepared iterator-range passes
  DevSchedule scratch;                                 // the one-off schedule of lpmp_compute_pass_custom
  int mode = -1;
  // the ticket lists of a pass count are device memory (C3, 32 passes: ~350 MB): the cache of built chains is bounded in BYTES
  // over all modes (the engine's rot_cache_limit; least recently used first), lpmp_chain_cache_bytes reports it
  // A chain whose kernel takes tickets ahead also holds one 64-byte descriptor per template ticket (DevChain::desc), two to three
  // times its other ticket arrays together: the headline's 20-pass template has 2.42 M tickets with 13.2 M dependencies, 155 MB of
  // descriptors beside 82 MB of ticket lists.  They are counted here before the cache makes room; a chain that fits the limit only without them
  // is built plain (rotation_chain)
  size_t rot_cache_bytes = 0;
  std::map<int, RotChain> rot_chain[LPMP_REPAM_COUNT];
  // (per form as well as per mode: the window and a TileSet are sized by block counts — [1]: the wide consume form, rot_wide)
  RotOrder rot_order[LPMP_REPAM_COUNT][2];
  // the block relations of a mode's joined passes with consume blocks (H, K, T) of PQ_WIDE_RECORDS records, beside the plan's own
  // (lpmp_plan::rot, every block the class's four): what a peer-minima launch in the wide consume form is planned from.  Built
  // with the plan's, while the host schedules still exist, and only where such a launch can come; not valid otherwise
  RotationInfo rot_wide[LPMP_REPAM_COUNT];
  // peer minima (kernels.hip, dense_pq_*_body): 32 doubles per factor, written by the W steps of a joined launch and read by its K / T
  // steps — never across calls (every call starts with H and W), so no upload invalidates it.  Allocated with the first eligible
  // joined launch, freed with the model; not part of the chain cache
  DevBuf<double> d_peerq;
  SpecBatch batch;

  // drop the joined-pass launches of a mode (or of all modes) and their order
  void release_rot_chains(int only_mode = -1) {
    for (int m = 0; m < LPMP_REPAM_COUNT; ++m) {
      if (only_mode >= 0 && m != only_mode) continue;
      for (auto& kv : rot_chain[m]) rot_cache_bytes -= std::min(rot_cache_bytes, kv.second.dev_bytes);
      rot_chain[m].clear();
      rot_order[m][0] = rot_order[m][1] = RotOrder();
    }
  }
  // every device schedule of the engine (built-in, partition, prepared iterator-range passes, the scratch one)
  template <class F>
  void for_each_schedule(F&& f) {
    for (int m = 0; m < LPMP_REPAM_COUNT; ++m) { for (int d = 0; d < 2; ++d) f(sched[d][m]); f(sched_pass[m]); f(sched_bf[m]); }
    for (int k = 0; k < 2; ++k) f(sched_part[k]);
    for (auto& c : custom) if (c) f(*c);
    f(scratch);
  }
  void release_primal() {
    d_primal.reset(); d_pinit.reset(); d_plinks.reset(); d_pw_unary.reset(); d_pcost.reset(); d_pbad.reset();
    have_primal = false; primal_unset_only = false; primal_t = 0; n_pinit = n_plinks = n_pprop = 0;
  }
  // the built-in schedules (everything but the caller's prepared iterator-range passes)
  void release_schedules() {
    for (int d = 0; d < 2; ++d) for (int m = 0; m < LPMP_REPAM_COUNT; ++m) sched[d][m].release();
    for (int m = 0; m < LPMP_REPAM_COUNT; ++m) { have_sched[m] = false; sched_pass[m].release(); sched_bf[m].release(); have_pass[m] = false; rotation_ok[m] = false; pass_chain_tried[m] = false; }
    for (int k = 0; k < 2; ++k) { sched_part[k].release(); have_part[k] = false; }
    release_rot_chains();
  }
};

}  // namespace host
}  // namespace lpmp

struct lpmp_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipStream_t capture_stream = nullptr;   // graphs are captured here (the caller's stream may be the legacy default stream, which cannot capture) and replayed on `stream`
  ModelState model;
  void release_model() { model = ModelState(); deep_note_given = false; }
  // this engine's block of device-written host words (from the pool, taken with the first upload) and the words in it
  char* pinned = nullptr; double* h_part = nullptr; unsigned long long* h_stale_n = nullptr; int* h_pbad = nullptr;
  bool use_lb_tracking = true;
  int64_t last_lb_recomputed = -1;   // factor bounds the last evaluation had to recompute (-1: none evaluated yet)
  bool primal_pass = false;       // the launches being issued belong to an ...AndPrimal pass
  bool want_rows = false;         // rows layout for the next upload (lpmp_set_rows_layout)
  int want_tab = LPMP_TABLES_F64; // table precision for the next upload (lpmp_set_table_precision)
  int inner_iterations = 5;                            // --innerIteration (reference LP_MP.h:590)
  bool use_fused = true;
  bool use_rotation = true;
  int rtype = 0;   // enum lpmp_reparametrization_type
  bool use_graph = true;
  bool use_chain = true;          // deep single-class schedules as one persistent launch (LPMP_NO_CHAIN=1: graph replay)
  DevBuf<int32_t> d_chain_abort; bool chain_ran = false;
  uint64_t rot_clock = 0;
  size_t rot_cache_limit = (size_t)2 << 30;   // bound of ModelState::rot_cache_bytes (default 2 GiB, LPMP_CHAIN_CACHE_MB)
  // ---- speculative passes (lpmp_set_speculation, include/lpmp_engine.h): the setting and the lifetime counters ----
  struct Spec {
    int max_depth = 0;                 // 0: off
    int64_t batches = 0, passes_launched = 0, passes_used = 0, rollbacks = 0, alloc_failures = 0;
  } spec;
  bool use_blocked_passes = true;     // LPMP_NO_BLOCKED_PASSES=1: the joined passes as one launch per step
  bool use_peer_minima = true;        // LPMP_NO_PEER_MINIMA=1: every joined launch in the old form (ModelState::d_peerq)
  int pq_lds = 1;                 // LPMP_PQ_LDS: the publishing records' form (kernels.hpp launch_chain)
  bool pq_scatter = true;         // LPMP_PQ_SCATTER: the three-table form publishes a table's row minima with a reduce-scatter (0: eight row all-reduces)
  // LPMP_PQ_AHEAD: 1 = a ticket of the shipped peer-minima form starts from a descriptor fetched during the ticket before
  // (kernels.hpp launch_chain), 0 = the kernels and tables without it, 2 = 1 with the consume records' old preload (measurements);
  // LPMP_PQ_DESC_INLINE: cap of the dependencies a descriptor holds inline (tests: 0 and 1 reach the path through dep[])
  int pq_ahead = 1, pq_desc_inline = TICKET_DESC_INLINE;
  int chain_max_wgs = 0;          // LPMP_CHAIN_MAX_WGS: cap of a chain launch's grid (tests, tracing); 0: what is resident at once
  int pq_hold = 3;                // LPMP_PQ_HOLD: tables such a record holds in registers, 3 or 2 (pq_lds 0: always 2, none parked)
  bool pq_wide = true;            // LPMP_PQ_WIDE=0: the consuming records one per wave, four per ticket, on the plan's own block relations
  // the ticket order of the peer-minima launches (rotation_chain): LPMP_PQ_TILES=0 the order every other launch takes (band order, or
  // tiles by the old rule), =T tiles of T blocks; LPMP_PQ_SUB / _SUBLAG / _SUBGAP: sub-bands per tile, their lag, the gap behind a predecessor (unset: the engine's own)
  int pq_tiles = -1, pq_sub = 0, pq_sublag = 0, pq_subgap = -1;
  int pq_min_passes = 12;         // LPMP_PQ_MIN_PASSES: calls of fewer passes keep the old order (rotation_chain)
  bool deep_note_given = false;                   // the one-line note about a schedule of many levels was printed
  RotSettings rot_opts;      // skewed ticket order (0 bands: from the table bytes per step); DESIGN.md 6 has the sweep
  // tiled ticket order of the joined passes (rotation_chain): LPMP_ROT_TILES=T forces tiles of T blocks per step, =0 forbids them;
  // unset: the engine's own choice (tiles of 1024 blocks where the band order is down to depth 2 or does not fit at all)
  int rot_tiles = 0; bool rot_tiles_set = false;
  bool timing = false;
  ClassTiming ct[KC_COUNT];
  struct Pending { hipEvent_t a, b; int cls; int64_t factors, receives, bytes; bool band = false, shift = false, shift_band = false; };   // band: sweep_diff_band_kernel; shift: a launch with a DIFF_SHIFT factor; shift_band: of those, sweep_diff_shift_band_kernel
  std::vector<Pending> pending;
  std::vector<hipEvent_t> event_pool;
  hipEvent_t get_event() {
    if (!event_pool.empty()) { hipEvent_t e = event_pool.back(); event_pool.pop_back(); return e; }
    hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); return e;
  }
  void drain_timing() {
    for (auto& p : pending) {
      HIP_CHECK(hipEventSynchronize(p.b));
      float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, p.a, p.b));
      ClassTiming& c = ct[p.cls];
      c.ms += ms; c.launches++; c.band_launches += p.band ? 1 : 0; c.shift_launches += p.shift ? 1 : 0; c.shift_band_launches += p.shift_band ? 1 : 0; c.factors += p.factors; c.receives += p.receives; c.bytes += p.bytes;
      event_pool.push_back(p.a); event_pool.push_back(p.b);
    }
    pending.clear();
  }
};

// ---- defined in engine.cpp ----------------------------------------------------------------------------------------------------
// (hidden: shared by the library's translation units, not exported from it)
#pragma GCC visibility push(hidden)
// copies between caller memory and the device, through the pinned staging buffer, waited for (STAGE_CHUNK bytes at a time)
constexpr size_t STAGE_CHUNK = (size_t)32 << 20;
void h2d(void* dst, const void* src, size_t bytes, hipStream_t stream);
void d2h(void* dst, const void* src, size_t bytes, hipStream_t stream);
template <class T, class V>
void fill_device(DevBuf<T>& dst, const V& src, hipStream_t stream) {
  dst.grow(src.size());
  h2d(dst, src.data(), src.size() * sizeof(T), stream);
}
// the `why` buffer of the lpmp_plan_*_info calls: after a refusal (rc != LPMP_OK) the text of lpmp_last_error, cut to why_n bytes
inline void copy_why(int rc, char* why, int why_n) {
  if (rc != LPMP_OK && why && why_n > 0) { std::strncpy(why, lpmp_last_error(), (size_t)why_n - 1); why[why_n - 1] = 0; }
}
// the steps a call goes through before it touches the model
void settle(lpmp_engine* e);                 // speculative passes: make the device state the caller's state
void check_chain(lpmp_engine* e);            // report an aborted chain run (waits for the stream)
void require_consts(const lpmp_engine* e);   // the constants are specified (no refused lpmp_upload_costs behind)
void rows_refresh(lpmp_engine* e);           // rows layout: packed duals -> rows, before anything computes on the rows
// the primal array: ensure_primal makes the one of the rounding code (UnsupportedError on a model it does not take),
// ensure_label_array that or the array of unset labels, upload_unset_primal writes "unset" into every slot of the one that exists
void ensure_primal(lpmp_engine* e);
void upload_unset_primal(lpmp_engine* e);
void ensure_label_array(lpmp_engine* e);
#pragma GCC visibility pop
