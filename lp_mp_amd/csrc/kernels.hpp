// kernels.hpp — the interface between the engine's host code (engine.cpp, prepared.cpp) and kernels.hip (device code and its launch
// wrappers): the one definition of every struct, constant and prototype that crosses the launch boundary.  Included by those files
// only (the host code through engine_state.hpp); the planner (plan.hpp and its sources) stays free of HIP.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan.hpp"

namespace lpmp {

// ---- limits of the generic kernels (engine.cpp checks every schedule against them) -----------------------------------
constexpr int GEN_MAXD = 512;            // generic kernel: max dual size / message length held in LDS per wave
constexpr int GEN_ADAPTIVE_SENDS = 64;   // adaptive send rule: sends per updated factor whose improvements a wave keeps

// ---- chain executor (kernels.hip: dependent levels inside one persistent launch) -------------------------------------
struct ChainArgs {
  const int32_t* dep_off;    // [n_tickets + 1]
  const int32_t* dep;        // predecessor tickets
  int32_t* done;             // [n_tickets]: epoch of the run that completed the ticket
  int32_t* next;             // ticket counter (zeroed before the launch)
  int32_t* abort_flag;
  const int32_t* tk_launch;  // [n_tickets]: launch (level x class range) the ticket belongs to
  const int32_t* tk_block;   // [n_tickets]: block of records inside that launch
  int32_t n_tickets;
  int32_t epoch;
  long long* trace;          // debugging (LPMP_CHAIN_TRACE): 8 slots of time stamps per ticket, 100 MHz; nullptr otherwise
  // joined passes (engine.cpp rotation_chain) with per-pass lower bounds: row r = the tracked bounds of all factors as they
  // are at the END OF PASS r + 1 of the call; a launch writes into the row its ChainLaunch::hist names (nullptr: no rows)
  double* lb_hist; int64_t hist_stride;
  // launches with CHAIN_LAUNCH_MAILBOX (chain_plan.cpp): rows of L granule pairs, see mailbox_put / mailbox_take
  unsigned long long* mailbox;
  // bound of every wait in ticks of s_memrealtime (100 MHz; engine.cpp: 20 s, LPMP_CHAIN_TIMEOUT_S).  Time, not a number of
  // polls: a device shared by several processes (N ranks of a smoke run on one GPU) serves a poll an order of magnitude
  // slower, and a count of polls that means seconds on an idle device was reached there by waits that were merely slow
  long long timeout_ticks;
  // PERIODIC ticket lists (the joined passes of lpmp_compute_pass(n), engine.cpp rotation_chain): the arrays above describe
  // a TEMPLATE — prologue tickets [0, per_begin), ONE period of per_len tickets, epilogue — and the launch executes the
  // period per_count times: ticket t of the launch is template ticket t - q * per_len of copy q = min((t - per_begin) /
  // per_len, per_count - 1) (0 in the prologue); its launch is the template's + q * per_launch_shift (every copy is a group
  // of as many steps later), its dependencies the template's + q * per_len, its bound row the template's + q * per_row_shift.
  // per_len == 0: plain lists.  Host work and device memory of an n-pass launch are then independent of n.
  int32_t per_begin, per_len, per_count, per_launch_shift, per_row_shift;
  // rows of lb_hist the launch may write (an n-pass call has n - 1 seams): a W step of a periodic template carries a row
  // even when, in a call that ends right behind it, it is the LAST step before T and has no seam behind it
  int32_t hist_rows;
  // ring > 0: done[] has `ring` slots, ticket t publishes {epoch, t / ring} into slot t % ring AFTER ticket t - ring has
  // published there (one more dependency of t), and a waiter accepts any generation >= the one it needs
  int32_t ring;
};
// tickets ahead (chain_dense_pq_ahead_kernel): one descriptor of TICKET_DESC_WORDS words per TEMPLATE ticket (plan.hpp
// ticket_descriptors) built with an inline cap of desc_inline, and the number of entries of the launch table, which that kernel
// keeps in LDS (at most PQ_AHEAD_MAX_LAUNCHES).  A kernel argument of its own and not a part of ChainArgs: every other chain kernel
// keeps its argument layout and with it its code.  form: 0 = not asked for (launch_chain: the other kernels); 1 = that kernel;
// 2 = that kernel with the consume records' send vectors preloaded as in the other kernels (LPMP_PQ_AHEAD=2: measurements)
struct ChainAhead { const int32_t* desc = nullptr; int32_t desc_inline = 0, n_launches = 0, form = 0; };
constexpr int PQ_AHEAD_MAX_LAUNCHES = 128;   // 5 KiB of LDS: calls of up to 63 passes as explicit lists, every periodic template
constexpr int CHAIN_GEN_BITS = 8;            // low bits of a ring slot: generation t / ring (< 256); the rest: the epoch
constexpr int CHAIN_ABORT_WORDS = 16;        // abort word + what the first wait that gave up was waiting for (kernels.hip, chain_abort)
// debugging (LPMP_LEVEL_TRACE, engine.cpp): time stamps of the first LEVEL_TRACE_MAX levels of a level-loop launch, 8 slots per level
constexpr int LEVEL_TRACE_MAX = 4000;
// one launch (a level x class range of records) as the chain kernels see it: absolute device pointers, so that tickets of
// one persistent launch may come from several schedules (the joined passes of lpmp_compute_pass(n), engine.cpp)
// pad: flags of the level loop (CHAIN_LAUNCH_LABEL_*), or for the joined passes of the dense chain kernel HIST_* | row << 2
struct ChainLaunch { const Op* packets; const UpdRec* recs; const Op* ops; int64_t count; int32_t stride, pad; };
static_assert(sizeof(ChainLaunch) == 40, "ChainLaunch layout");
// Which tracked bounds of a launch also go to a row of ChainArgs::lb_hist.  n joined passes are H, W, (K, W)^(n-1), T
// (DESIGN.md 4): the state "after pass i" is never in memory as a whole — K_i holds the last receives of pass i AND the
// first sends of pass i + 1 — but every factor's bound at that moment is known to exactly one record:
//   HIST_END  (a W step)  the updated factor's bound at the end of the record (it is not touched again in this pass)
//   HIST_MID  (a K step)  the updated factor's bound after its receives, before its sends, and the bound of every
//                         pairwise factor it receives from, right after that receive
constexpr int HIST_END = 1, HIST_MID = 2;

// ---- records of the other kernels --------------------------------------------------------------------------------------
// shared classes: a table of the pool — offset relative to the const base pointer, dims
struct ShTableDesc { int64_t off; int32_t d0, d1; };
// lower bound / primal cost of one factor (reference LP::LowerBound, LP_MP.h:1507-1518), in factor order
struct LbRec { int64_t dual_off; int64_t const_off; int32_t d0, d1; int32_t kind_flags; int32_t pad; };
// rows layout: one dense pairwise factor's place in the packed arrays and in the rows (kernels.hip, rows_copy_kernel)
struct RowRec { int64_t dual_off, const_off, row_off; int32_t d0, d1; };
// table precision: one dense table's place in the chunk of doubles being narrowed and in the float buffer (narrow_tables_kernel)
struct NarrowRec { int64_t src_off, dst_off, n; int32_t factor, pad; };
// new costs on a planned model: one listed vector factor of lpmp_set_vectors (its place in the packed duals, its row of the source)
struct SetVecRec { int64_t dual_off, src_row; int32_t len, factor; };
// ... one listed pairwise factor of lpmp_set_constants: its row of the source and every place the sweep kernels read its constants
// from, in 8-byte units relative to the const base pointer (the engine's other allocations are addressed that way, too, so an
// offset may be negative): dst, and with `two` set dst2 for a second copy of doubles.  f32: the factor is a DENSE one whose table
// is stored as floats, starting at dst
struct SetConstRec { int64_t dst, dst2, src_row; int32_t len, factor, f32, two; };
// ... and one piece of the pairwise message vectors lpmp_zero_pairwise_duals clears (device dual offset, at most ZERO_RUN_MAX doubles)
struct ZeroRec { int64_t dual_off, len; };
constexpr int64_t ZERO_RUN_MAX = 8192;
// conditional rounding from the duals (decode_kernel; plan.hpp, DecodePlan): one decoded unary, and one of its links — the pairwise
// factor's duals and constants (relative to the two base pointers, as everywhere), its kind and dims, the unary's side in it, the
// unary on the other side and that unary's level (the launch of level l counts, in the initial sweep, the links with level < l)
struct DecodeRec { int64_t dual_off; int32_t d0, link_begin, n_links, factor; };
struct DecodeLink { int64_t peer_dual, peer_const; int32_t kind, pd0, pd1, side, other, level; };
static_assert(sizeof(DecodeRec) == 24 && sizeof(DecodeLink) == 40, "decode record layout");
constexpr int DECODE_GROUP_MAX = 32;     // up to this many labels a lane group of 4 / 8 / 16 / 32 lanes takes a unary, above it a wave
constexpr int DECODE_CHUNK = 4 * 64;     // labels a wave holds in registers at a time (more: chunk by chunk, the links read again)
constexpr int DECODE_ALL = 1;            // launch flag: every link counts (a refinement sweep); otherwise only those of a lower level
// prepared read-outs (lpmp_readout_*): one listed vector factor — its place in the packed duals (vector factors live
// there under every layout), the row of the destination it fills, its label count; for the beliefs its links (DecodeLink records
// whose `other` / `level` are unused) in the order of its MESSAGE LIST, the order in which a sweep receives
struct ReadoutRec { int64_t dual_off, row; int32_t d0, factor, link_begin, n_links; };
static_assert(sizeof(ReadoutRec) == 32, "read-out record layout");
constexpr int READOUT_GROUP_MAX = DECODE_GROUP_MAX;   // beliefs: a lane group per unary up to this many labels, a wave above (the decode's split)
constexpr int READOUT_CHUNK = DECODE_CHUNK;           // ... and the labels a wave holds in registers at a time
// path moves (lpmp_path_moves; DESIGN.md 8, path_moves_kernel): a path is a run of nodes.  A node: its place in the packed duals
// (vector factors live there under every layout), its label count, its links in ascending message index, and the path edge to the
// PREVIOUS node — constants, kind and second dimension of that pairwise factor and the side the previous node has in it
// (edge_kind < 0: the first node) — and where its back-pointers go in the scratch buffer: d0 entries at byte back_off, one byte
// each when the previous node has at most 256 labels (back_wide == 0), two otherwise.  A link: the message vector of the node's
// side (device dual offset), the pairwise factor's constants, kind and second dimension, the node's side, the unary on the other
// side with its label count, and on_path for a path edge (only the message vector is added then)
struct PathRec { int64_t node_begin; int32_t n_nodes, pad; };
struct PathNode { int64_t dual_off, edge_const, back_off; int32_t d0, factor, link_begin, n_links, edge_kind, edge_d1, edge_prev_side, back_wide; };
struct PathLink { int64_t vec_off, peer_const; int32_t kind, pd1, side, other, od, on_path; };
static_assert(sizeof(PathRec) == 16 && sizeof(PathNode) == 56 && sizeof(PathLink) == 40, "path record layout");
constexpr int PATH_WAVE_MAX = 64;        // a wave per path while no node of it has more labels (four paths per workgroup), a workgroup above
static_assert(PATH_MAX_LABELS <= GEN_MAXD, "path moves hold a vector of f in LDS");
// forest moves (lpmp_forest_moves; DESIGN.md 8, forest_up_kernel / forest_down_kernel): a node of a tree.  As a PathNode: its place
// in the packed duals, its label count, its links (PathLink records in ascending message index; on_path marks the tree edges, to
// the parent and to the children alike).  The tree edge to the PARENT: constants, kind and second dimension of that pairwise factor,
// the side THIS node has in it, the parent's factor and label count dq (parent < 0: a root).  Its row g of dq doubles starts at
// element g_off of the scratch of rows, its dq back-pointers at byte back_off of the scratch of back-pointers: one byte each while
// this node has at most 256 labels (back_wide == 0), two otherwise.  Its children: n_children entries from child_begin of the
// child table, each the g_off of a child's row (of d0 doubles), in ascending message index of this node's message into the edge
struct ForestNode { int64_t dual_off, edge_const, g_off, back_off; int32_t d0, factor, link_begin, n_links, edge_kind, edge_d1, edge_side, back_wide, dq, parent, child_begin, n_children; };
static_assert(sizeof(ForestNode) == 80, "forest record layout");
// moving label windows (lpmp_move_windows): one listed unary — its place in the packed duals, its label count (at most
// MOVE_MAX_LABELS: a wave holds a whole vector in registers), its row of delta / cost_old / cost_new, and its links in message-list
// order: the message vector of its side in the pairwise factor (device dual offset) ...
struct MoveRec { int64_t dual_off; int32_t d0, factor, link_begin, n_links, row, pad; };
struct MoveLink { int64_t vec_off; };
// ... and one DIFF_SHIFT factor adjacent to a listed unary: where the sweep kernels read its shift (the third word of its cell) and
// the scalar of the constants the cell is gathered from, both in 8-byte units relative to the const base pointer as in SetConstRec,
// and the rows of the unaries on its two sides (-1: no unary there, or one that is not listed: delta 0)
struct MoveShiftRec { int64_t cell, packed; int32_t left_row, right_row, factor, pad; };
static_assert(sizeof(MoveRec) == 32 && sizeof(MoveShiftRec) == 32, "window record layout");
static_assert(MOVE_MAX_LABELS == GEN_MAXD, "window moves hold a vector in the registers of one wave (plan.hpp)");
constexpr int MOVE_DELTA_MAX = 1 << 20;               // |delta| of a move: a host value beyond it is refused, a device value saturated

// ---- launch wrappers (kernels.hip) -------------------------------------------------------------------------------------
// The bool ones return false when there is no kernel for the request (each says when, at its definition).
void launch_sweep(int kclass, const UpdRec* recs, const Op* ops, double* dual, const double* cdata, const int32_t* tabs,
                  double* lb, int32_t* primal, const int32_t* pw_unary, int64_t first, int64_t count, int flags, hipStream_t s);
bool launch_sweep_packed(int kclass, const Op* packets, const UpdRec* recs, const Op* ops, int stride, double* dual, const double* cdata,
                         double* lb, int32_t* primal, int64_t count, int flags, hipStream_t s);
bool launch_sweep_shared(int kclass, const Op* packets, const UpdRec* recs, const Op* ops, int stride, double* dual, const double* cdata,
                         double* lb, int32_t* primal, int64_t count, int flags, const ShTableDesc* desc, const int32_t* tabs, int n_tabs, hipStream_t s);
// band: the launch's LevelRange::diff_band or diff_shift_band (cdata then holds a band word in front of every D)
// shift: the launch's LevelRange::diff_shift (DIFF_SHIFT peers, plain DIFF ones beside them)
// neither: sweep_diff_kernel; band: sweep_diff_band_kernel; shift: sweep_diff_shift_kernel; both: sweep_diff_shift_band_kernel
void launch_sweep_diff(bool band, bool shift, const UpdRec* recs, const Op* ops, double* dual, const double* cdata, double* lb, int32_t* primal, int64_t first, int64_t count,
                       int flags, hipStream_t s);
// peerq != nullptr: the launches carry CHAIN_LAUNCH_PQ_* roles (joined passes with peer minima; KC_DENSE_32 on f64 tables only)
// pq_lds: the publishing records' form (LPMP_PQ_LDS): 1 park their first table in LDS, 0 request both of the first pair again
// pq_hold: tables a publishing record holds in registers (LPMP_PQ_HOLD) when pq_lds is 1: 3 = three and one parked, no table
// requested twice; 2 = two and one parked, table 1 of a record with four receives requested again.  pq_lds 0 ignores it
// pq_scatter: the three-table form's publish on the column side of a table (LPMP_PQ_SCATTER): true = a reduce-scatter inside the
// 16-lane row (chain_dense_pq_scatter_kernel), false = eight row all-reduces (chain_dense_pq_kernel<32, 3, 1, *>); the two-table forms ignore it
// pq_wide: the consuming records' form (LPMP_PQ_WIDE): true = two records per wave, PQ_WIDE_RECORDS per ticket — the launches'
// H / K / T blocks must have been planned with that many records (order.cpp plan_rotation_chain, consume_gpb)
// ahead (LPMP_PQ_AHEAD; form != 0): chain_dense_pq_ahead_kernel, the scatter form with wide consume records whose tickets start from
// a descriptor fetched during the ticket before (pq_ahead_applies says which forms have it; false for the others)
// max_wgs > 0 (LPMP_CHAIN_MAX_WGS): no chain launch has more workgroups.  Safe for any value >= 1: a ticket waits for lower tickets
// only, and those are held by workgroups that are running
bool launch_chain(int kclass, int flags, const ChainArgs& ca, const ChainLaunch* launches, double* dual, const double* cdata,
                  const int32_t* tabs, double* lb, int32_t* primal, hipStream_t s, double* peerq = nullptr, int pq_lds = 1, bool pq_wide = false, int pq_hold = 2, bool pq_scatter = false,
                  const ChainAhead& ahead = ChainAhead(), int max_wgs = 0);
inline bool pq_ahead_applies(int pq_lds, int pq_hold, bool pq_wide, bool pq_scatter, int n_launches) {
  return pq_lds != 0 && pq_hold == 3 && pq_wide && pq_scatter && n_launches <= PQ_AHEAD_MAX_LAUNCHES;
}
// grid and resident workgroups per CU of that launch; num_regs / scratch_bytes: what hipFuncGetAttributes reports for its kernel
// (numRegs, localSizeBytes; -1 when the query fails)
unsigned chain_pq_grid(int pq_lds, int pq_hold, bool pq_wide, bool pq_scatter, int n_tickets, int* per_cu, int* num_regs = nullptr, int* scratch_bytes = nullptr,
                       int pq_ahead = 0, int max_wgs = 0);   // pq_ahead: ChainAhead::form
bool launch_level_loop(int kclass, int flags, const ChainLaunch* launches, int n_launches, double* dual, const double* cdata,
                       const int32_t* tabs, double* lb, hipStream_t s);
void debug_set_level_trace(long long* p);
void launch_primal_init(const PrimalInit* list, int64_t n, int32_t* primal, hipStream_t s);
void launch_primal_propagate(const PrimalLink* links, int64_t n, int32_t* primal, hipStream_t s);
// one level of a decode sweep: records [first, first + count) of recs, all with at most `width` labels when width <= DECODE_GROUP_MAX
// (a lane group of the next power of two >= max(width, 4) per unary), any label count otherwise (a wave per unary)
void launch_decode(const DecodeRec* recs, const DecodeLink* links, const double* dual, const double* cdata, int32_t* primal,
                   int64_t first, int64_t count, int width, int level, int flags, int tab32, hipStream_t s);
// prepared read-outs: dst[row] = label slot of the record's factor; row `row` of dst (rows dst_stride doubles apart) = its theta
// (width: the longest listed vector, which picks the lane group); ... = its belief, for records [first, first + count) that all have
// at most `width` labels when width <= READOUT_GROUP_MAX.  Entries of a row beyond the factor's label count are not written
void launch_readout_labels(const ReadoutRec* recs, int64_t n, const int32_t* primal, int32_t* dst, hipStream_t s);
void launch_readout_vectors(const ReadoutRec* recs, int64_t n, int width, const double* dual, double* dst, int64_t dst_stride, hipStream_t s);
void launch_readout_beliefs(const ReadoutRec* recs, const DecodeLink* links, const double* dual, const double* cdata, double* dst,
                            int64_t dst_stride, int64_t first, int64_t count, int width, int tab32, hipStream_t s);
// path moves: paths [first, first + count) of one group, all of one form — wide == 0: no node has more than PATH_WAVE_MAX labels
// (a wave per path), wide != 0: a workgroup per path.  Exact dynamic programming over each path given the labels of all other
// unaries; writes the back-pointers into `back` and the new labels of the paths' nodes into primal
void launch_path_moves(const PathRec* paths, const PathNode* nodes, const PathLink* links, const double* dual, const double* cdata,
                       int32_t* primal, unsigned char* back, int64_t first, int64_t count, int wide, int tab32, hipStream_t s);
// forest moves, one height level of one group: the nodes list[first, first + count) all of one form — wide == 0: neither the node
// nor its parent has more than PATH_WAVE_MAX labels (a wave per node), wide != 0: a workgroup per node.  f = node cost + the
// children's rows; a non-root node stores its row and back-pointers, a root writes its label into primal
void launch_forest_up(const int32_t* list, const ForestNode* nodes, const int64_t* child_g, const PathLink* links, const double* dual, const double* cdata,
                      int32_t* primal, double* rows, unsigned char* back, int64_t first, int64_t count, int wide, int tab32, hipStream_t s);
// ... and one depth level >= 1: primal[node] = back_node[primal[parent]]
void launch_forest_down(const int32_t* list, const ForestNode* nodes, int32_t* primal, const unsigned char* back, int64_t first, int64_t count, hipStream_t s);
void launch_primal_check(const PrimalLink* links, int64_t n, const int32_t* primal, int* bad, hipStream_t s);
void launch_primal_cost(const LbRec* recs, const double* dual, const double* cdata, const int32_t* primal, double* out, int64_t count, int tab32, hipStream_t s);
void launch_lb_collect_stale(const double* lb, int64_t n, int32_t* list, unsigned long long* counter, hipStream_t s);
// tab32 (here and in launch_primal_cost): nonzero when the DENSE tables are stored as floats (the sweep kernels: SWEEP_TAB32)
void launch_factor_lb_list(const LbRec* recs, const double* dual, const double* cdata, double* out, const int32_t* list, int64_t count, int tab32, hipStream_t s);
void launch_factor_lb(const LbRec* recs, const double* dual, const double* cdata, double* out, int64_t count, int tab32, hipStream_t s);
bool launch_dense_lb(int L, const LbRec* recs, const double* dual, const double* cdata, double* out, int64_t first, int64_t count, int tab32, hipStream_t s);
void launch_sum_stage(const double* in, double* out, int64_t n, int64_t per_block, int64_t n_blocks, hipStream_t s);
void launch_synth_fill(double* out, int64_t n, uint64_t seed, uint64_t first, hipStream_t s);
void launch_rows_copy(const RowRec* recs, int64_t n, const double* cdata, double* dual, double* rows, int what, hipStream_t s);
void launch_shared_cells(double* cells, int64_t n, const double* cdata, hipStream_t s);
// table precision: n tables of src (doubles) become floats in dst; strict: refuse entries that are not exactly floats; *bad keeps the
// lowest factor index with a refused entry (the caller sets it to INT32_MAX first)
void launch_narrow_tables(const NarrowRec* recs, int64_t n, const double* src, float* dst, int strict, int* bad, hipStream_t s);
// new costs on a planned model: theta of the listed vector factors := / += rows of src (and their tracked bounds become NaN);
// the listed runs of the dual array := +0.0
void launch_set_vectors(const SetVecRec* recs, int64_t n, const double* src, int64_t src_stride, double* dual, double* lb, int accumulate, hipStream_t s);
void launch_zero_pairwise(const ZeroRec* recs, int64_t n, double* dual, hipStream_t s);
// constants of the listed pairwise factors := rows of src, written to every place of the record (float tables narrowed), their
// tracked bounds NaN.  The check launch writes nothing but *bad: the lowest factor index whose float table would refuse an entry of
// its row, by the rule of launch_narrow_tables (the caller sets it to INT32_MAX first)
void launch_set_constants_check(const SetConstRec* recs, int64_t n, const double* src, int64_t src_stride, int strict, int* bad, hipStream_t s);
void launch_set_constants(const SetConstRec* recs, int64_t n, const double* src, int64_t src_stride, double* cdata, double* lb, hipStream_t s);
// moving label windows: theta and every linked message vector of record k := the same vector gathered through
// g(x) = clamp(x + delta[row], 0, d0 - 1), in place; cost_old / cost_new (both or neither; rows cost_stride doubles apart) add
// cost_new[row][x] - cost_old[row][g(x)] to theta where the two differ.  The shifts: shift := clamp(int(shift) + delta[left_row]
// - delta[right_row], -2^30, 2^30) at both places of record i when the two deltas differ.  The tracked bounds of all of them: NaN
void launch_move_windows(const MoveRec* recs, const MoveLink* links, int64_t n, const int32_t* delta, double* dual, double* lb,
                         const double* cost_old, const double* cost_new, int64_t cost_stride, hipStream_t s);
void launch_move_shifts(const MoveShiftRec* recs, int64_t n, const int32_t* delta, double* cdata, double* lb, hipStream_t s);
// primal state on the device.  set_labels: label slot of record i's factor := src[row] (device array), unset (the dimension) for a
// value outside [0, d0 - 1].  carry_labels: the label slot x < d0 of record i's factor := clamp(x - delta[row], 0, d0 - 1), the delta
// saturated as in launch_move_windows; unset slots stay.  factor_lb_list_dev: launch_factor_lb_list with the count read from
// *counter on the device (max_count: the most it can be, sizes the fixed grid of at most LB_LIST_DEV_BLOCKS workgroups).  sum_final:
// *dst = constant + part[0] + ... + part[n_part - 1] added in that order by one thread, or +inf when bad != nullptr and *bad != 0
constexpr int64_t LB_LIST_DEV_BLOCKS = 2048;
void launch_set_labels(const ReadoutRec* recs, int64_t n, const int32_t* src, int32_t* primal, hipStream_t s);
void launch_carry_labels(const MoveRec* recs, int64_t n, const int32_t* delta, int32_t* primal, hipStream_t s);
void launch_factor_lb_list_dev(const LbRec* recs, const double* dual, const double* cdata, double* out, const int32_t* list,
                               const unsigned long long* counter, int64_t max_count, int tab32, hipStream_t s);
void launch_sum_final(const double* part, int64_t n_part, double constant, const int* bad, double* dst, hipStream_t s);

}  // namespace lpmp
