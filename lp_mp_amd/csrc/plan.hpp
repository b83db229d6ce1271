// plan.hpp — host-side analysis of a flat LP_MP model: per-factor message lists, update ordering,
// send weights / receive masks for every reparametrisation mode, and the level schedule the HIP
// sweep kernels execute.  Pure C++17 (no HIP): the same code runs in the CPU-only test container.
//
// Reference behaviour restated here (paths relative to /root/reference):
//   message lists  include/factors_messages.hxx:3339-3365, :3402-3419, storage order :2081-2119, :2030-2041
//   FactorUpdated  include/factors_messages.hxx:3125-3140
//   ordering       include/LP_MP.h:730-797, include/topological_sort.hxx:100-144
//   weights        include/LP_MP.h:1232-1415 (anisotropic), :1086-1154 (anisotropic2), :1422-1449 (uniform),
//                  :1489-1505 (full receive mask)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/lpmp_model.h"

namespace lpmp {

// a model that is valid in the reference but beyond a size limit of the device kernels (include/lpmp_engine.h,
// lpmp_upload_model): the C ABI answers LPMP_ERR_UNSUPPORTED; every other std::runtime_error of the planner is a malformed
// model or argument (LPMP_ERR_INVALID)
struct UnsupportedModel : std::runtime_error { using std::runtime_error::runtime_error; };

struct MsgEntry {          // one element of FactorContainer::get_messages()
  int32_t msg;
  int32_t adjacent;
  uint8_t role;            // 0: this factor is the message's left factor, 1: right
  uint8_t sends, receives, adj_sends, adj_receives;
};

template <class T>
struct Csr {
  std::vector<int64_t> off{0};
  std::vector<T> data;
  int64_t rows() const { return (int64_t)off.size() - 1; }
};

// Device-side records (plain structs shared with kernels.hip) -----------------------------------
enum OpCode : int32_t { OP_UP = 0, OP_LABELING = 1, OP_MINNORM = 2 };
constexpr int32_t OP_HAS_IMPROVEMENT = 1 << 12;   // Op::info: the message op defines send_message_to_*_improvement
// Op::info, only in the PACKET copy of an op of a chain launch with CHAIN_LAUNCH_MAILBOX (chain_plan.cpp): the
// message vector travels through the chain's mailbox.  A send: peer_const = mailbox row the new vector is also written to;
// a receive: the bits of omega = mailbox row (int64) the OTHER side's vector is polled from instead of the dual array.
constexpr int32_t OP_MAILBOX = 1 << 13;

struct alignas(16) UpdRec {   // one updated factor
  int64_t dual_off;   // own dual start
  int64_t const_off;  // own const start (pairwise) or -1
  int32_t d0, d1;     // own dims (vector: d0 = n, d1 = 0)
  int32_t op_begin;   // first op
  int16_t n_recv, n_send;
  int32_t factor;
  int32_t kind_flags; // own kind (bits 0-3) | flags << 4
};
static_assert(sizeof(UpdRec) == 48, "UpdRec layout");

struct alignas(16) Op {       // one active receive or send
  int64_t peer_dual;  // peer dual start
  int64_t peer_const; // peer const start (pairwise peer), or offset of the match table in tab_data (labeling)
  double omega;       // send weight (receives: 1.0)
  int32_t info;       // opcode | role<<4 | side<<5 | right_implicit_origin<<6 | peer_implicit_origin<<7 | peer_kind<<8 | has_improvement<<12
  int32_t pd0;        // peer dim0
  int32_t pd1;        // peer dim1 (dense pairwise peer) / n_left of the table (labeling)
  int32_t peer;       // peer factor index (slot of its tracked lower bound)
  int32_t len;        // message length (= dim of the left factor's variable)
  int32_t pad;
};
static_assert(sizeof(Op) == 48, "Op layout");

// kernel classes: which kernel runs an updated factor
enum KClass : int32_t {
  KC_GENERIC = 0,
  KC_DENSE_4, KC_DENSE_8, KC_DENSE_16, KC_DENSE_32,
  KC_POTTS_4, KC_POTTS_8, KC_POTTS_16, KC_POTTS_32,
  // any label count <= the padded width (runtime dims, also rectangular d0 x d1 tables for the dense classes)
  KC_DENSE_V4, KC_DENSE_V8, KC_DENSE_V16, KC_DENSE_V32,
  KC_POTTS_V4, KC_POTTS_V8, KC_POTTS_V16, KC_POTTS_V32,
  // one wave per unary, dense tables of any dims up to BIG_MAX_LABELS streamed in 16-row blocks
  KC_DENSE_BIG,
  // one LANE per updated factor: tiny factors of any kind (every dual size / message length <= SMALL_MAXD)
  KC_SMALL,
  // UPDATED dense pairwise factors (`right` / `full` schedules: the factor pulls its unaries in and sends both
  // min-marginals back), dims <= the padded width, at most PW_MAX_OPS ops: packet form, one read of the table
  KC_PW_4, KC_PW_8, KC_PW_16, KC_PW_32,
  // unaries whose active messages all go to SHARED pairwise factors (LPMP_F_PAIRWISE_SHARED): run-time label counts and
  // rectangular tables up to the padded width; the launch's distinct tables are staged in LDS once per workgroup
  KC_SHARED_4, KC_SHARED_8, KC_SHARED_16, KC_SHARED_32,
  // unaries whose active messages all go to DIFF or DIFF_SHIFT pairwise factors (LPMP_F_PAIRWISE_DIFF, ..._DIFF_SHIFT, any mix), 2 ... BIG_MAX_LABELS labels, any
  // number of ops: one wave per unary, op by op; a receive builds scale * D in LDS and reads no table from memory
  KC_DIFF,
  KC_COUNT
};
constexpr int BIG_MAX_LABELS = 512;
// A DIFF vector D of n entries is BANDED when all entries outside an index range [lo, hi] equal, to the bit, D[0] (below lo) or
// D[n - 1] (above hi) and the range has at most n / DIFF_BAND_DIV entries (a truncated potential).  A KC_DIFF launch
// whose receives all reference banded vectors runs sweep_diff_band_kernel: the window and two tail terms instead of all pairs.
constexpr int DIFF_BAND_DIV = 4;
constexpr bool diff_band_rule(int64_t lo, int64_t hi, int64_t n) { return (hi - lo + 1) * DIFF_BAND_DIV <= n; }
// A DIFF_SHIFT receive (dims d0 x d1, pool vector D of any n entries, shift s) expands D over i = a - b + d1 - 1 in [0, ne),
// ne = d0 + d1 - 1, as D[clamp(i - off, 0, n - 1)], off = d1 - 1 - s: the band of D moved by off and clipped to [0, ne), the clamp
// continuing the two tails.  The shift moves the band and never widens it, so the rule reads the width of D's OWN band against ne
// and stays a function of structure and pool values: diff_band_rule(lo, hi, ne).  A launch with a DIFF_SHIFT peer whose receives
// all pass it runs sweep_diff_shift_band_kernel (a plain DIFF peer beside them is the case n = ne, off = 0: its own rule).
constexpr int SMALL_MAXD = 8;
constexpr int PW_MAX_OPS = 6;
constexpr bool kc_is_pw(int kclass) { return kclass >= KC_PW_4 && kclass <= KC_PW_32; }
constexpr bool kc_is_shared(int kclass) { return kclass >= KC_SHARED_4 && kclass <= KC_SHARED_32; }
// tables one launch of a shared class may reference (the kernel's LDS budget: per table two slots of width x width doubles —
// the table and its transpose —, 64 KiB at 32 labels beside 8 KiB of slabs: two workgroups per CU in the worst case); a record
// that would take its launch beyond it goes to another launch of the class (plan.cpp, classify: split by table set)
constexpr int SHARED_MAX_TABLES = 4;
// launches the shared records of one level and width may be split into by table set; what no group takes runs on the generic class
constexpr int SHARED_MAX_GROUPS = 32;
// lanes-per-vector width of a packed fast class (0: generic / streaming class)
constexpr int kc_width(int kclass) {
  if (kclass >= KC_PW_4 && kclass <= KC_PW_32) return 4 << (kclass - KC_PW_4);
  if (kclass >= KC_SHARED_4 && kclass <= KC_SHARED_32) return 4 << (kclass - KC_SHARED_4);
  return (kclass == KC_GENERIC || kclass >= KC_DENSE_BIG) ? 0 : 4 << ((kclass - 1) % 4);
}
constexpr bool kc_is_dense(int kclass) { return (kclass >= KC_DENSE_4 && kclass <= KC_DENSE_32) || (kclass >= KC_DENSE_V4 && kclass <= KC_DENSE_V32); }
constexpr bool kc_is_var(int kclass) { return kclass >= KC_DENSE_V4 && kclass <= KC_POTTS_V32; }
// the unary classes of the packed kernels: every launch of one has packets or indirect records (LevelRange::stride != 0)
constexpr bool kc_is_packed(int kclass) { return kclass >= KC_DENSE_4 && kclass <= KC_POTTS_V32; }

struct LevelRange {            // one kernel launch: a range of UpdRec indices of one level and class
  int32_t kclass; int64_t begin, end;
  int32_t level = 0;                            // 1-based dependent step this launch belongs to
  int64_t n_recv = 0, n_send = 0, bytes = 0;   // active receives / sends / algorithmic bytes of the range
  // packed form (fast classes with few ops per factor): factor i of the range has its UpdRec in slot
  // pk_begin + i*stride of Schedule::packets and its ops in the following slots -> one coalesced load, no
  // dependent rec -> ops hop.  stride < 0: indirect mode (below).  stride 0: an op-by-op class (generic, streaming, lane per factor).
  int32_t stride = 0; int64_t pk_begin = 0;
  int32_t max_dim = 0;                          // largest label count of any vector or table side the launch's records touch
  // shared classes: the distinct shared tables (indices into the model's pool) the launch's records reference
  int32_t n_sh = 0; int32_t sh_tab[SHARED_MAX_TABLES] = {};
  // class diff: every receive of every record references a banded vector (cleared by LPMP_NO_DIFF_BAND): the banded kernel
  bool diff_band = false;
  // class diff: a record of the launch has a DIFF_SHIFT peer (LPMP_F_PAIRWISE_DIFF_SHIFT): one of the two shifted kernels, never
  // sweep_diff_band_kernel — structure, so new pool values (Plan::refresh_diff_band) leave it alone
  bool diff_shift = false;
  // class diff, diff_shift: every receive of every record passes the shifted rule (diff_band_rule above against the receive's
  // d0 + d1 - 1; cleared by LPMP_NO_DIFF_BAND): sweep_diff_shift_band_kernel, otherwise sweep_diff_shift_kernel.  Pool values
  // and structure decide it, never a shift
  bool diff_shift_band = false;
  // class diff: the launch's row of Schedule::diff_tab_off — the pool entries diff_band was decided from (-1: another class)
  int32_t diff_row = -1;
};
constexpr int PK_MAX_OPS = 8;                 // packets hold at most this many ops per factor
// launches whose factors have more ops than that (but at most this many: the LDS slab of a lane group) run the
// same kernels in INDIRECT mode (LevelRange::stride < 0): record from recs[], then all its ops from ops[] in one
// coalesced load — two dependent hops instead of one per op
constexpr int pk_indirect_cap(int labels) { return labels >= 16 ? 32 : labels >= 8 ? 16 : 8; }
// the dense classes at 16 labels hold 64 ops: 50 KB of LDS per workgroup of 16 records = three workgroups per CU, the
// occupancy the dense kernel's registers allow anyway — so the hubs of a random graph of mean degree 10 stay on the packed
// kernel (as launches of their own on the streaming kernel they cost C4 1.5 of 13.4 ms per pass, profiles/r03_c4b_*).
// The Potts kernels (more waves per SIMD) keep the smaller slab.
constexpr int pk_dense_cap(int labels) { return labels == 16 ? 64 : pk_indirect_cap(labels); }
constexpr int pk_class_cap(int kclass) { return kc_is_dense(kclass) ? pk_dense_cap(kc_width(kclass)) : pk_indirect_cap(kc_width(kclass)); }   // (shared classes: the smaller slab)
constexpr int32_t UPD_PRELOAD_OK = 1 << 16;   // UpdRec::kind_flags: no send targets a vector a receive writes
constexpr int32_t UPD_PRIMAL = 1 << 17;       // UpdRec::kind_flags: the factor type has COMPUTE_PRIMAL_SOLUTION

// kernel flags of the sweep kernels
constexpr int SWEEP_RESIDUAL = 1;   // --reparametrizationType residual
constexpr int SWEEP_NT = 4;         // host-side selector: the model is far larger than the caches -> non-temporal variants
constexpr int SWEEP_ADAPTIVE = 8;   // --reparametrizationType adaptive (generic kernels only)
constexpr int SWEEP_TAB32 = 16;     // the DENSE pairwise tables are stored as floats (lpmp_set_table_precision): the f32 kernels, and the
                                    // table reads of the generic kernels
// bits 8-11: streaming dense class — LDS per wave sized for ceil(max label count of the launch / 64) * 64 labels (0: BIG_MAX_LABELS)
constexpr int SWEEP_BIGDIM_SHIFT = 8, SWEEP_BIGDIM_MASK = 15 << SWEEP_BIGDIM_SHIFT;
constexpr int sweep_bigdim_flags(int max_dim) { return max_dim <= 0 ? 0 : (((max_dim + 63) / 64) << SWEEP_BIGDIM_SHIFT) & SWEEP_BIGDIM_MASK; }
constexpr int SWEEP_PRIMAL = 2;     // UpdateFactorPrimal (reference factors_messages.hxx:2332-2373): factors of a
                                    // COMPUTE_PRIMAL type round their label from the state after the receives

// primal rounding (engine.cpp / kernels.hip): one unary-pairwise message, and one lazily initialised factor
struct PrimalLink { int32_t u, p, side, dim; };   // left (vector) factor, right (pairwise) factor, side, label count of u
struct PrimalInit { int32_t f, a, b, pad; };      // primal_ of factor f when unset: (a, b)

// Chain executor (kernels.hip): the launches of a deep schedule as ONE persistent launch.  A ticket = one workgroup's
// block of records of one launch; dep = the tickets holding the predecessors of its records (the last earlier update
// of every factor a record touches).  Tickets are numbered in level order, so a dependency always has a lower number.
struct ChainLaunchHost { int64_t rec_begin, count, pk_begin; int32_t stride, ticket0; int32_t flags = 0; };   // flags: CHAIN_LAUNCH_LABEL_OPS
constexpr int32_t CHAIN_LAUNCH_LABEL_PAIRED = 2;  // ... and in every record send j goes to the peer receive j came from (each message received, then sent)
// dense chain launches: message vectors between dependent records travel as tagged granules (kernels.hip, mailbox); the
// dependencies they cover are not in dep[] any more.  Bit 30: the low bits of ChainLaunch::pad belong to the joined passes.
constexpr int32_t CHAIN_LAUNCH_MAILBOX = 1 << 30;
// joined passes with peer minima (kernels.hip, dense_pq_*_body): the role of a step, in ChainLaunch::pad above the bound row —
// a W step publishes per edge what the neighbour's next receive computes from the table, the other steps consume it
constexpr int32_t CHAIN_LAUNCH_PQ_PUBLISH = 1 << 28, CHAIN_LAUNCH_PQ_CONSUME = 1 << 29;
constexpr int32_t CHAIN_LAUNCH_PQ_MASK = CHAIN_LAUNCH_PQ_PUBLISH | CHAIN_LAUNCH_PQ_CONSUME;
constexpr int PEER_MINIMA_MAX_OPS = 4;          // receives / sends per record the peer-minima bodies hold in registers
// the sends of a record that may go to the mailbox = the sends (and forwarded receives) the mailbox form of the dense body
// holds in registers (kernels.hip: KS, NFW)
constexpr int MAILBOX_SENDS = 4;
constexpr int32_t CHAIN_LAUNCH_LABEL_OPS = 1;   // level loop: every record a vector factor whose ops are labeling messages with it on the left, <= 8 receives and <= 8 sends, no two of a kind on one peer
// level loop: a CHAIN_LAUNCH_LABEL_OPS launch of at most LL_STAGE_RECS records is staged in LDS by the wave that runs ahead
// (kernels.hip, StagedLevel: LL_STAGE_OPS op slots per record = 8 receives + 8 sends); a larger one reads its records from memory
constexpr int LL_STAGE_RECS = 16, LL_STAGE_OPS = 16;
struct ChainPlan {
  bool valid = false;
  int32_t kclass = 0;                       // the one kernel class of the schedule
  std::vector<ChainLaunchHost> launches;    // parallel to Schedule::launches
  std::vector<int32_t> tk_launch;           // [n_tickets]
  std::vector<int32_t> tk_block;            // [n_tickets]: block of records inside that launch
  std::vector<int32_t> dep_off, dep;        // CSR over tickets
  bool banded = false;                      // tickets in Infinity-Cache order: the tables are read with plain loads
  bool level_loop = false;                  // many tiny levels of a generic class: ONE workgroup walks the launches (kernels.hip)
  int64_t mailbox_rows = 0;                 // message vectors that travel through the mailbox (rows of mailbox_width granule pairs)
  int64_t mailbox_receives = 0;             // receives that poll a row
  int32_t mailbox_width = 0;
};
// records one workgroup of the packed kernels takes (256 threads / lanes per record)
constexpr int GENERIC_BLOCK_RECORDS = 4, SMALL_BLOCK_RECORDS = 64;   // sweep_generic_kernel<64> / <1> (kernels.hip asserts them)
constexpr int BIG_BLOCK_RECORDS = 4;          // sweep_dense_big_kernel: one wave per record (kernels.hip asserts it)
constexpr int kc_block_records(int kclass) {
  if (kclass == KC_GENERIC) return GENERIC_BLOCK_RECORDS;
  if (kclass == KC_SMALL) return SMALL_BLOCK_RECORDS;
  const int w = kc_width(kclass);
  if (w == 0) return 0;
  return (kc_is_dense(kclass) || kc_is_shared(kclass)) ? (w == 32 ? 4 : 256 / w) : 256 / w;   // dense / shared: G = 64 lanes at 32 labels, else one lane per label
}
constexpr bool kc_chain_capable(int kclass) { return kc_is_packed(kclass) || kclass == KC_GENERIC || kclass == KC_SMALL; }
constexpr int64_t CHAIN_MIN_LAUNCHES = 9;   // shorter schedules run as plain launches

// vectors of op records are hundreds of megabytes at the headline size and every element is written right after the
// allocation: default-initialise (= leave alone) instead of zero-filling them first
// contiguous chunks of [0, n) on a few threads (host analysis of models with millions of factors; plan.cpp has the same for
// its own loops): f(begin, end); exceptions are rethrown on the caller's thread
template <class F>
inline void parallel_blocks(int64_t n, int64_t min_per_thread, F&& f) {
  const unsigned hw = std::thread::hardware_concurrency();
  const int64_t nt = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, hw ? hw : 1), n / std::max<int64_t>(1, min_per_thread)));
  if (nt <= 1) { f((int64_t)0, n); return; }
  std::vector<std::thread> th;
  std::vector<std::exception_ptr> err((size_t)nt);
  th.reserve((size_t)nt);
  auto work = [&](int64_t t) { try { f(n * t / nt, n * (t + 1) / nt); } catch (...) { err[(size_t)t] = std::current_exception(); } };
  int64_t started = 0;
  try {
    for (; started < nt - 1; ++started) th.emplace_back(work, started);
  } catch (...) {}                                   // (a thread could not be started: the caller's thread takes the remaining chunks)
  for (int64_t t = started; t < nt; ++t) work(t);
  for (auto& x : th) x.join();
  for (auto& e : err) if (e) std::rethrow_exception(e);
}

template <class T>
struct default_init_allocator : std::allocator<T> {
  template <class U> struct rebind { using other = default_init_allocator<U>; };
  default_init_allocator() = default;
  template <class U> default_init_allocator(const default_init_allocator<U>&) noexcept {}
  template <class U> void construct(U* p) { ::new (static_cast<void*>(p)) U; }
  template <class U, class... A> void construct(U* p, A&&... a) { ::new (static_cast<void*>(p)) U(std::forward<A>(a)...); }
};
using OpVec = std::vector<Op, default_init_allocator<Op>>;

struct Schedule {             // executable form of one (factor list, omega, mask) sweep
  std::vector<UpdRec> recs;   // sorted by (level, kclass)
  OpVec ops;
  OpVec packets;                      // packed launches: [UpdRec | Op x (stride-1)] per factor
  std::vector<LevelRange> launches;   // in execution order
  int64_t n_levels = 0;
  int64_t n_recv = 0, n_send = 0;     // active receives / sends = message updates per sweep
  int64_t alg_bytes = 0;              // algorithmic HBM bytes per sweep (DESIGN.md accounting)
  // deep schedules: one chain plan per kernel class (classes between which no dependency runs are independent
  // sequences), the launches of the remaining classes stay plain launches (indices into `launches`)
  std::vector<ChainPlan> chains;
  std::vector<int32_t> plain_launches;
  // per KC_DIFF launch (LevelRange::diff_row, CSR): the distinct pool entries that decide its kernel — those of its receives, of its
  // sends where it has no receive.  All a schedule keeps of the pool's VALUES is diff_band of those launches, and with this list
  // Plan::refresh_diff_band sets it again from new values without the records and ops (which the engine does not keep on the host).
  // diff_tab_ne, beside every entry of diff_tab: the smallest d0 + d1 - 1 among those receives (sends) of the launch that reference
  // the pool entry — what the shifted rule holds the width of the entry's band against (LevelRange::diff_shift_band)
  std::vector<int32_t> diff_tab_off, diff_tab, diff_tab_ne;
};

// Conditional rounding from the duals (lpmp_decode_primal): the structure of a decode in one direction.  Every vector
// factor is a decoded unary; pi = Plan::order[direction] restricted to them.  level(u) = 1 + max level(v) over the neighbours v
// earlier in pi (1 without any): two neighbours never share a level and a neighbour later in pi has a higher one, so the
// unaries of one level are independent and level by level equals the sequential walk — for the initial sweep (neighbours of a
// LOWER level count) and for a refinement sweep (all count: lower levels hold this sweep's label, higher ones the previous one's).
struct DecodeEdge { int32_t p, side, other; };   // pairwise factor, the unary's side in it, the unary on the other side
struct DecodePlan {
  std::string why;                       // "" or why the model is refused (names the lowest offending factor); nothing else is filled then
  int32_t bad_factor = -1;
  std::vector<int32_t> unaries, level;   // in pi; level is 1-based
  std::vector<int64_t> edge_off;         // CSR over `unaries`: the edges of a unary in ascending message index
  std::vector<DecodeEdge> edges;
  int32_t n_levels = 0;
};

// Path moves (lpmp_path_moves): the structure of a path set.  Groups of paths of VECTOR factors; consecutive members
// of a path are joined by exactly one pairwise factor (the path edge), found here.  Per entry (a member of a path, in the caller's
// order): the edge to the PREVIOUS member with the side the previous member has in it, and the member's links in ascending
// message index — on_path marks the one or two that are path edges, whose table the recursion reads instead of a line of it.
constexpr int32_t PATH_MAX_LABELS = 512;
struct PathLinkPlan { int32_t p, side, other, on_path; };   // pairwise factor, the member's side in it, the unary on the other side
struct PathPlan {
  std::string why;                       // "" or why the set is refused as unsupported (names the lowest offending listed unary)
  int32_t bad_factor = -1;
  std::vector<int64_t> group_off, path_off;
  std::vector<int32_t> unaries;
  std::vector<int32_t> edge, edge_prev_side;   // per entry; -1 / 0 for the first member of a path
  std::vector<int64_t> link_off;         // CSR over the entries
  std::vector<PathLinkPlan> links;
  int64_t n_path_edges = 0, n_off_path_links = 0, longest = 0;
  int32_t max_labels = 0;
};

// Forest moves (lpmp_forest_moves): the structure of a forest set.  Groups of VECTOR factors with a parent each (a factor
// index, -1 for a root); a child and its parent are joined by exactly one pairwise factor (the tree edge), found here, and no other
// pairwise factor joins two members of a group.  Per entry, in the caller's order: the parent's entry, the tree edge with the side
// the ENTRY has in it, the links in ascending message index (tree: 0 = a cost line, 1 = the edge to the parent, 2 = to a child),
// the children (entries) in ascending message index of the entry's message into the tree edge, the height (0 for a leaf) and the
// depth (0 for a root).
struct ForestLinkPlan { int32_t p, side, other, tree; };
struct ForestPlan {
  std::string why;                       // "" or why the set is refused as unsupported (names the lowest offending listed unary)
  int32_t bad_factor = -1;
  std::vector<int64_t> group_off;
  std::vector<int32_t> unaries, parent, parent_entry;
  std::vector<int32_t> edge, edge_side;  // per entry; -1 / 0 for a root
  std::vector<int64_t> link_off;         // CSR over the entries
  std::vector<ForestLinkPlan> links;
  std::vector<int64_t> child_off;        // CSR over the entries
  std::vector<int32_t> children;
  std::vector<int32_t> height, depth;
  std::vector<int32_t> group_height;     // per group: the highest height (-1: an empty group)
  int64_t n_trees = 0, n_tree_edges = 0, n_off_tree_links = 0;
  int32_t max_height = 0, max_labels = 0;
};
// Moving label windows (lpmp_move_windows): the structure of a window set, from the structure alone.  The listed unaries
// (every VECTOR factor without a list), the links of each in message-list order, and the DIFF_SHIFT factors next to them with the
// row of the unary on either side (-1: not listed).
constexpr int MOVE_MAX_LABELS = 512;       // a listed unary's label count: a wave holds a whole vector in registers (kernels.hpp)
struct WindowLink { int32_t p, side; };
struct WindowPair { int32_t p, left_row, right_row; };
struct WindowPlan {
  std::string why;                       // "" or why the set is refused as unsupported (names the lowest offending listed unary)
  int32_t bad_factor = -1;
  std::vector<int32_t> factors;
  std::vector<int64_t> link_off;        // CSR over `factors`
  std::vector<WindowLink> links;
  std::vector<WindowPair> pairs;        // in the order the listed unaries meet them
  int32_t max_labels = 0;
};
// The unary on each side of every pairwise factor, from all unary-pairwise messages: side_unary[2 p + s], and how many messages
// name that side (saturating at 2).  What path sets, forest sets and the forest cover judge a unary by (Plan::move_obstacle)
struct PairSides { std::vector<int32_t> side_unary; std::vector<uint8_t> side_count; };

struct Plan {
  // copied structure (no cost data)
  int32_t n_ftypes = 0, n_mtypes = 0, n_tables = 0;
  std::vector<uint8_t> ftype_primal;
  std::vector<lpmp_msg_type> mtypes;
  std::vector<int64_t> tab_off;
  std::vector<int32_t> tab_data, tab_nleft;
  int64_t nf = 0, nm = 0;
  std::vector<int32_t> f_type, f_dim0, f_dim1;
  std::vector<uint8_t> f_kind, f_flags;
  std::vector<int64_t> f_coff, f_doff;   // [nf+1]
  // shared pairwise tables (LPMP_F_PAIRWISE_SHARED): the pool, copied (a handful of small tables), and every factor's table
  // (-1: neither a SHARED nor a DIFF / DIFF_SHIFT factor; a DIFF factor's entry is its 1 x (dim0 + dim1 - 1) vector, a DIFF_SHIFT factor's a 1 x n vector)
  int32_t n_shared = 0;
  std::vector<int64_t> sh_off; std::vector<int32_t> sh_dim0, sh_dim1; std::vector<double> sh_data;
  std::vector<int32_t> f_table;
  // per pool entry a DIFF or DIFF_SHIFT factor references: the band [sh_lo, sh_hi] of its vector (diff_band below).  sh_banded:
  // whether the plain rule holds (0 / 1; -1: no DIFF factor references the entry — a DIFF_SHIFT factor does not count, its rule
  // depends on the receive: diff_launch_shift_banded).  sh_shift_ref: a DIFF_SHIFT factor references the entry
  std::vector<int32_t> sh_lo, sh_hi; std::vector<int8_t> sh_banded; std::vector<uint8_t> sh_shift_ref;
  bool no_diff_band = false;     // LPMP_NO_DIFF_BAND set when the plan was built: no launch gets LevelRange::diff_band
  std::vector<int32_t> m_type, m_left, m_right;
  double constant = 0;
  // derived
  std::vector<int64_t> fm_off;
  std::vector<MsgEntry> fm;
  std::vector<uint8_t> updated;
  std::vector<int32_t> order[2], upd[2];
  Csr<double> omega[2][LPMP_REPAM_COUNT];
  Csr<uint8_t> mask[2][LPMP_REPAM_COUNT];
  bool have[LPMP_REPAM_COUNT] = {false, false, false, false};
  int max_dual = 1;
  // LP::put_in_same_partition pairs (call order) and what construct_factor_partition derives from them
  std::vector<int32_t> part_pairs;
  struct SegList { std::vector<int32_t> f; Csr<double> om; Csr<uint8_t> mk; };   // a factor list with the weights of a pass over it
  struct Partition {
    bool valid = false;
    std::vector<int64_t> off; std::vector<int32_t> f;          // partitions (updated factors only), CSR
    std::vector<SegList> fwd, bwd, push_fwd, push_bwd, ov_fwd, ov_bwd;
  } part;
  bool any_batch = false;        // some message op has a static batch send (lpmp_msg_flags)
  bool force_generic = false;    // schedule every update on the generic kernels (adaptive sends)
  // device memory a schedule's mailbox may take (16 bytes per label and mailbox send; C3 row-major: 2 GB): the engine sets it
  // from the free memory of its device, and a class whose mailbox would not fit is planned with completion flags only
  // (-1: no limit)
  int64_t mailbox_budget_bytes = -1;
  // dense pairwise tables are stored as floats on the device (lpmp_set_table_precision / lpmp_plan_set_table_precision): 4 instead
  // of 8 bytes per entry in the byte accounting of every schedule made from now on — classes, levels and records are the same
  bool tables_f32 = false;
  // Engine-private placement of factors on the device (engine.cpp, rows layout): where a factor's constants start relative
  // to the const base pointer and its duals relative to the dual base pointer, in doubles — possibly in ANOTHER allocation
  // (the kernels only ever form base + offset).  Empty: the packed offsets f_coff / f_doff.  Sizes always come from f_*.
  std::vector<int64_t> dev_coff, dev_doff;
  int64_t coff(int64_t f) const { return dev_coff.empty() ? f_coff[f] : dev_coff[f]; }
  int64_t doff(int64_t f) const { return dev_doff.empty() ? f_doff[f] : dev_doff[f]; }

  // throws std::runtime_error on invalid input (the reference throws too, LP_MP.h:458)
  void build(const lpmp_model& m);
  // New VALUES for the pool (same entries, offsets and dims; packed as lpmp_model.sh_data).  A NaN entry is refused with nothing
  // changed.  Of the plan, only sh_data and the band of every entry a DIFF or DIFF_SHIFT factor references (sh_lo / sh_hi /
  // sh_banded) read a pool value; of a schedule, only diff_band and diff_shift_band of its KC_DIFF launches: refresh_diff_band sets
  // those again, for the launches of a schedule or of any copy of them (tabs_off / tabs / tabs_ne: the schedule's diff_tab_off /
  // diff_tab / diff_tab_ne).  Returns whether a launch changed.
  void set_shared_pool(const double* values);
  // the banded kernel for a KC_DIFF launch: only if every one of these pool entries (Schedule::diff_tab) holds a banded vector
  bool diff_launch_banded(const int32_t* tabs, int64_t n) const;
  // ... and for one with a DIFF_SHIFT peer: only if the band of every entry passes the rule against its ne (Schedule::diff_tab_ne)
  bool diff_launch_shift_banded(const int32_t* tabs, const int32_t* ne, int64_t n) const;
  bool refresh_diff_band(std::vector<LevelRange>& launches, const std::vector<int32_t>& tabs_off, const std::vector<int32_t>& tabs,
                         const std::vector<int32_t>& tabs_ne) const;
  // (without the ne row a launch with a DIFF_SHIFT factor goes to the full shifted kernel, which is correct for every vector)
  bool refresh_diff_band(std::vector<LevelRange>& launches, const std::vector<int32_t>& tabs_off, const std::vector<int32_t>& tabs) const {
    return refresh_diff_band(launches, tabs_off, tabs, std::vector<int32_t>());
  }
  void ensure_weights(int mode);
  void anisotropic_weights(const int32_t* list, int64_t n, Csr<double>& om, Csr<uint8_t>& mk) const;
  // one sweep: a factor list with one omega row and one receive-mask row per listed factor
  struct Segment { const int32_t* factors; int64_t n; const int64_t* om_off; const double* om; const int64_t* mk_off; const uint8_t* mk; };
  // turn a sequence of sweeps into levels/records/ops; fuse: fold back-to-back updates of one factor (plan.cpp)
  // chains = false: a schedule of exactly three levels (the shape whose consecutive passes the engine joins into its own
  // persistent launch, engine.cpp rotation_chain) gets no chain plan of its own — a third of the planning time at the
  // headline size for lists the joined launch never reads
  // levels_only (optional): only the dependent level of every update is wanted — filled ([sum of the segments' n]; 0 for an update
  // that becomes no record: no active message and no primal to round) and nothing else is built (a third of the work)
  void make_schedule(const std::vector<Segment>& segs, bool fuse, Schedule& out, bool chains = true, std::vector<int32_t>* levels_only = nullptr) const;
  void make_schedule(const int32_t* factors, int64_t n, const int64_t* om_off, const double* om,
                     const int64_t* mk_off, const uint8_t* mk, Schedule& out) const;
  int64_t row_sends(int32_t f) const { return n_row_sends[(size_t)f]; }       // entries of f's message list that send / receive
  int64_t row_receives(int32_t f) const { return n_row_receives[(size_t)f]; }
  std::vector<int32_t> n_row_sends, n_row_receives;
  // LP::construct_factor_partition / construct_overlapping_factor_partition (reference LP_MP.h:1717-1843)
  void ensure_partition();
  // the iterator-range passes of compute_partition_pass (rtype 2, LP_MP.h:1932-1963) or
  // compute_overlapping_partition_pass (rtype 3, :1966-2051; without the plain sweeps that follow it), in order
  void partition_pass_segments(int rtype, int inner_iterations, std::vector<Segment>& out);
  // CallSendMessages' batch rule (reference factors_messages.hxx:2709-2726) as the weights the individual sends get
  void effective_send_weights(int32_t f, const double* omega, double* w) const;
  // why the adaptive send rule cannot run this model ("" if it can)
  std::string adaptive_obstacle() const;
  // Structure of lpmp_decode_primal in `direction` (0 / 1).  Supported: every message is LPMP_M_UNARY_PAIRWISE and every
  // pairwise factor has exactly one of them on each side, from two different unaries.  Otherwise DecodePlan::why says what the
  // lowest offending factor is (a factor of a message of another kind; a pairwise factor with a side that has no unary or two,
  // or with one unary on both sides)
  DecodePlan decode_plan(int direction) const;
  // Structure of a path set (include/lpmp_engine.h, lpmp_path_set_create): group_off [n_groups + 1] in paths, path_off [n_paths + 1]
  // in entries, unaries [entries].  Throws std::runtime_error (LPMP_ERR_INVALID) naming the entry, with `who` in front; a set the
  // move does not take comes back with PathPlan::why set.  Order of the checks: offsets, indices and kinds, duplicates inside a
  // group; then the unsupported shapes; then the path edges (they are read off the supported shape)
  PathPlan path_plan(int64_t n_groups, const int64_t* group_off, const int64_t* path_off, const int32_t* unaries, const std::string& who) const;
  // Structure of a forest set (include/lpmp_engine.h, lpmp_forest_set_create): group_off [n_groups + 1] in entries, unaries and
  // parent [entries].  Throws std::runtime_error (LPMP_ERR_INVALID) naming the entry, with `who` in front; a set the move does
  // not take comes back with ForestPlan::why set.  Order of the checks: offsets, indices and kinds, duplicates inside a group,
  // parents, cycles; then the unsupported shapes (those of path_plan); then the tree edges and the pairwise factors that would
  // close a cycle or join two trees
  ForestPlan forest_plan(int64_t n_groups, const int64_t* group_off, const int32_t* unaries, const int32_t* parent, const std::string& who) const;
  // Structure of a window set (include/lpmp_engine.h, lpmp_window_set_create): n listed factors, or factors == nullptr for every VECTOR
  // factor.  Throws std::runtime_error (LPMP_ERR_INVALID) naming the entry: out of range, not a VECTOR factor, listed twice; a set
  // the move does not take comes back with WindowPlan::why set, naming the lowest listed factor with an obstacle
  WindowPlan window_plan(int64_t n, const int32_t* factors, const std::string& who) const;
  // what the unsupported-shape check of path_plan / forest_plan reads, and the check itself on VECTOR factor u: "" or what is
  // wrong with it (a message that is not unary-pairwise with u on the left; an adjacent pairwise factor without exactly one
  // unary on each side from two different unaries; more than PATH_MAX_LABELS labels — `move` is the word the message uses)
  PairSides pair_sides() const;
  std::string move_obstacle(int32_t u, const PairSides& ps, const char* move) const;
};

// The band of a difference vector D of n entries, by the BITS of the doubles (-0.0 and +0.0 differ): lo = the first index whose
// entry is not D[0] (n if there is none), hi = the last index >= lo whose entry is not D[n - 1] (lo - 1 if there is none).  Every
// entry below lo is D[0], every entry above hi is D[n - 1], and hi - lo + 1 >= 0 is the width.  model.diff_band (Python) is the
// same statement.
void diff_band(const double* D, int64_t n, int32_t* lo, int32_t* hi);

// graph.cpp: an order of all factors with the updated ones colour by colour (rank[f] = position; returns the number of colours)
int32_t suggest_order(const Plan& p, uint64_t seed, int32_t* rank);
// graph.cpp: a cover of the unaries a forest move takes (Plan::move_obstacle finds none) by groups that each induce a forest,
// every tree rooted at a centre (include/lpmp_engine.h, lpmp_plan_suggest_forests).  group_off in entries; returns the number of
// VECTOR factors left out
struct ForestCover { std::vector<int64_t> group_off; std::vector<int32_t> unaries, parent; int64_t n_left_out = 0; };
ForestCover suggest_forests(const Plan& p, int64_t max_groups);

// ---- order.cpp: ticket orders of the Infinity-Cache chain launches ------------------------------------------------------------
// A skewed order of the blocks of consecutive steps: new_of[base[s] + j] = ticket of block j of step s (base: the steps' blocks in
// step order), tk_step / tk_block = the inverse; group_begin = first ticket of every group of `depth` steps, and N at the end.
struct TicketOrder { std::vector<int32_t> tk_step, tk_block, new_of; std::vector<int64_t> group_begin; };
// Skewed band order: step s (nb[s] blocks) is cut into `bands` bands, block j in band floor(j * bands / nb[s]); inside a group of
// `depth` steps, band b of the group's d-th step comes at time b + lag * d: tickets sorted by (band + lag * d, d, block)
void band_order(const std::vector<int64_t>& nb, int bands, int lag, int depth, TicketOrder& o);

// Joined passes as ONE persistent launch (chain executor with a skewed ticket order): what the expansion
// for n passes needs of the two fused schedules.  Templates: H, W, T = the three steps of forward+backward, K = the middle
// step of backward+forward; n passes = H, W, (K, W)^(n-1), T.
struct RotationInfo {
  bool valid = false;
  int kclass = 0, gpb = 1;       // gpb: records per block of the W template (the class's own)
  int consume_gpb = 1;           // ... of the H, K and T templates (one common count: the tiled order needs equal block counts there)
  struct Tmpl { int sched; LevelRange lr; int32_t nb; int64_t factors, recv, bytes; };   // sched: 0 forward+backward, 1 backward+forward
  Tmpl t[4];                                                   // H, W, K, T
  // predecessors of a step's blocks: kind 0 W after [H]; 1 K after [W, H]; 2 W after [K, W]; 3 K after [W, K];
  // 4 T after [W, K]; 5 T after [W, H].  (delta, block): the block of the step delta steps earlier
  std::vector<int64_t> off[6]; std::vector<int8_t> delta[6]; std::vector<int32_t> block[6];
  // every factor's bound at a pass seam is known to a W record (its own, at the end) or a K record (its own after the
  // receives, or as the pairwise peer of one of its receives): then a joined launch can emit one bound row per pass
  bool hist_ok = false;
  // how far AHEAD in a step's block list a steady-state block's predecessors of the step before lie, as a fraction of the
  // list (a W x H grid in a 2-colour order: one grid row, 1 / H): what the lag of the skewed ticket order has to cover before any slack
  double reach = 0;
  // peer minima: the STRUCTURE allows the W records to publish, per edge, the minima the K / T record at the other
  // end would compute from the table, so that K / T read no table (the engine adds: f64 tables, packed layout, switch not off);
  // peer_minima_why: "" or the first obstacle (LPMP_ROT_VERBOSE prints it)
  bool peer_minima = false;
  std::string peer_minima_why = "not a joined pass";
};
// fb, bf: forward+backward and backward+forward of a mode whose passes join (engine.cpp plan_rotation), nf factors; not valid
// unless H, W, K, T are one packed launch each of one chain-capable class
// consume_gpb: records per block of the H, K, T templates (0: the class's own, as W) — the wide consume form of the peer-minima
// kernel takes PQ_WIDE_RECORDS; dependencies, reach and block counts follow every template's own block size
constexpr int PQ_WIDE_RECORDS = 8;
RotationInfo plan_rotation_chain(const Schedule& fb, const Schedule& bf, int64_t nf, int consume_gpb = 0);

// ---- chain_plan.cpp: the chain plans of a deep schedule, from its records, launches and packets ------------------------------
// the knobs of chain planning (chain_settings_from_env: read on every make_schedule that reaches chain planning)
struct ChainSettings {
  int64_t chain_min = CHAIN_MIN_LAUNCHES;       // LPMP_CHAIN_MIN: the smallest number of launches that makes a class a chain
  bool chain_all = false;                       // LPMP_CHAIN_ALL != 0: tickets for the generic / lane-per-factor classes too, no heavy-launch exit
  bool no_level_loop = false;                   // LPMP_NO_LEVEL_LOOP set
  bool no_blocked_passes = false;               // LPMP_NO_BLOCKED_PASSES set: no banded order
  int64_t band_min_bytes = (int64_t)64 << 20;   // LPMP_BAND_MIN_BYTES: bytes of a step with table reads that count for the banded order
  bool band_min_set = false;                    // ... set: every model counts as bigger than the Infinity Cache
  int64_t band_bytes = (int64_t)16 << 20;       // LPMP_BAND_BYTES (>= 1): algorithmic bytes per band
  int64_t heavy_bytes = (int64_t)256 << 20;     // LPMP_CHAIN_HEAVY_BYTES: mean bytes per launch from which a long schedule stays plain (<= 0: never)
  bool no_mailbox = false;                      // LPMP_NO_MAILBOX set: every hand-over through a completion flag
  bool verbose = false;                         // LPMP_ROT_VERBOSE set: level-loop diagnostics on stderr
};
ChainSettings chain_settings_from_env();
// the update sequence of a schedule as make_schedule saw it: per update its factor, the update whose record holds its ops (itself
// unless it was folded into an earlier one), its omega and receive-mask rows
struct UpdateView { int64_t n; const int32_t* factor; const int32_t* owner; const double* const* om; const uint8_t* const* mk; };
// rec_upd: the update each record of `out` stands for.  Fills out.chains and out.plain_launches, and marks the mailbox ops of
// out.packets (OP_MAILBOX); throws std::runtime_error on an inconsistent plan
void plan_chains(const Plan& p, const UpdateView& seq, const std::vector<int32_t>& rec_upd, const ChainSettings& cs, Schedule& out);

// the window of the band order: LPMP_ROT_BANDS / _LAG / _DEPTH (bands 0: from the table bytes per step; *_set: given, used as they are)
struct RotSettings { int bands = 0, lag = 3, depth = 4; bool lag_set = false, depth_set = false; };
// fits = false: even depth 2 cannot hold the window in the Infinity Cache
struct RotGeometry { int bands = 1, lag = 3, depth = 4; bool fits = true; double reach_bytes = 0; };
RotGeometry rot_geometry(const RotSettings& rs, const RotationInfo& ri);

// tiles of about T blocks of the W and K steps (w, k: tile of every block; n tiles); delayed[sd]: share of a steady-state step's
// blocks that run later than their own tile's phase, sd steps into a group; depth: the group depth that follows from it
// (make_tiles fills delayed[0 .. 7], which is what the depth follows from; extend_tile_delays fills the rest, so that groups of 12 and
// 16 steps can be judged by the same figures: both were slower than 8 on the headline grid, EXPERIMENTS.md T, and no rule picks them)
constexpr int TILE_STEPS_MAX = 16;
struct TileSet { int T = 0; std::vector<int32_t> w, k; int32_t n = 0; double radius = 0; double delayed[TILE_STEPS_MAX] = {}; int depth = 2; bool delays_extended = false; };
TileSet make_tiles(const RotationInfo& ri, int T);
void extend_tile_delays(const RotationInfo& ri, TileSet& ts);

// The geometry of a peer-minima launch (engine.cpp rotation_chain; EXPERIMENTS.md T).  step_bytes: what a step of that form moves —
// W: tables + vectors + the minima it writes, H / K / T: vectors + the minima they read (RotationInfo::t[].bytes still counts a table
// per K / T receive).  use: the tables of a W step exceed the Infinity Cache.  tile_blocks (the T of make_tiles) follows from
// tile_bytes of a W step, sub from the W tickets a sub-band should hold.  peer_minima_geometry(ri, T > 0): for tiles of T blocks.
struct PqGeometry { bool use = false; int tile_blocks = 0, depth = 8, sub = 1, sub_lag = 1, sub_gap = 0; int64_t step_bytes[4] = {0, 0, 0, 0}; double tile_bytes = 0, w_blocks_per_tile = 0; };
PqGeometry peer_minima_geometry(const RotationInfo& ri, int tile_blocks = 0);
// share of a W step's table reads that is expected to come from HBM: the first W step of a group of `depth` steps, and the delayed
// blocks of the others (their tile's phase is long over)
double peer_minima_hbm_share(const TileSet& ts, int depth);
// tiled order of n joined passes: in a group of `depth` steps a block runs in the phase of its own tile or the latest phase of its
// predecessors in the group; tickets sorted by (phase, step, block)
void tiled_order(const RotationInfo& ri, int n, const TileSet& ts, int depth, TicketOrder& o);
// the same with the band order's skew over the tiles: every tile cut into `sub` sub-bands in block order, all sub-bands one list in
// tile order, sub-band b of the group's sd-th step at time b + lag * sd, a block never before time(predecessor) + gap; tickets by
// (time, step, block); sub <= 1: tiled_order
void skewed_tile_order(const RotationInfo& ri, int n, const TileSet& ts, int depth, int sub, int lag, int gap, TicketOrder& o);

// the order of a joined-pass launch: band order (bands, lags from `lag` to max(16, 2 lag), depth) or, with tiles, the tiled order
// sub > 1 (tiles only): the skewed tiled order, sub sub-bands per tile at a lag of sub_lag times between consecutive steps
struct JoinedOrder { int bands = 1, lag = 3, depth = 4; const TileSet* tiles = nullptr; int sub = 1, sub_lag = 1, sub_gap = 0; };
struct JoinedTables {
  std::vector<int32_t> tk_launch, tk_block, dep_off, dep;   // ticket -> step, block; dependencies (CSR over tickets)
  std::vector<int> step_tmpl;                               // per step: its template (0 H, 1 W, 2 K, 3 T)
  std::vector<int32_t> step_row;                            // per step: the per-pass bound row its launch writes (-1: none)
  int32_t per_begin = 0, per_len = 0, ring = 0;             // periodic template: the period's tickets, slots of the flag ring
  int lag = 0;                                              // the lag the band order was built with
  int sub = 1;                                              // the sub-bands the tiled order was built with (1: the plain tiled order)
};
// the tables of n joined passes (periodic: the template of n passes whose group 2 is the period; the depth must be even) — ""
// or why the passes stay one launch per step; log (or nullptr): progress lines.  ri must be valid.
std::string joined_pass_tables(const RotationInfo& ri, const JoinedOrder& ord, int n, bool periodic, JoinedTables& out, FILE* log);
// One fixed-size descriptor per TEMPLATE ticket (the peer-minima kernel with tickets ahead, kernels.hip chain_loop_roles_ahead): what
// a ticket otherwise collects from tk_launch, tk_block, dep_off and dep in dependent round trips, as one 64-byte record that 16 lanes
// fetch with one word each.  Word TD_LAUNCH: the template launch; TD_BLOCK: the block; TD_NDEPS: the dependency count; TD_REST:
// the position in dep[] where the dependencies that are not inline continue, dep_off[t] + min(count, cap); TD_DEPS ...: the first
// min(count, cap) predecessor tickets, -1 behind them.  cap is clamped to [0, TICKET_DESC_INLINE].  The periodic arithmetic (copy,
// shifts, ring predecessor) stays in the kernel: a descriptor describes a template ticket.
constexpr int TICKET_DESC_WORDS = 16, TD_LAUNCH = 0, TD_BLOCK = 1, TD_NDEPS = 2, TD_REST = 3, TD_DEPS = 4;
constexpr int TICKET_DESC_INLINE = TICKET_DESC_WORDS - TD_DEPS;
std::vector<int32_t> ticket_descriptors(const std::vector<int32_t>& tk_launch, const std::vector<int32_t>& tk_block, const std::vector<int32_t>& dep_off,
                                        const std::vector<int32_t>& dep, int cap = TICKET_DESC_INLINE);
// hist[c] = tickets with c dependencies (the last entry: that many or more)
std::vector<int64_t> ticket_dep_histogram(const std::vector<int32_t>& dep_off, int max_count);

}  // namespace lpmp
