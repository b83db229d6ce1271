/*
 * lpmp_engine.h — C ABI of the MI355X sweep engine (liblpmp_engine.so).
 *
 * This is the drop-in boundary for ONE path of pawelswoboda/LP_MP: the dual block-coordinate-ascent
 * sweep LP<FMC>::ComputePass and the dual bound LP<FMC>::LowerBound.  The reference's plug-in API is
 * compile-time C++ (FactorContainer / MessageContainer / LP<FMC> templates); the host-side mirrors
 * (lp_mp_amd/include/LP_gpu.hxx for C++, lp_mp_amd/lp.py for Python) keep that surface and talk to the
 * device through the functions below.  Plain pointers and sizes only; no exceptions cross this
 * boundary; every function returns 0 on success or a negative lpmp_status and sets
 * lpmp_last_error().  The host-side mirrors re-throw std::runtime_error, the type the reference throws
 * (reference include/LP_MP.h:458, include/topological_sort.hxx:115).
 *
 * Conventions (mirroring how the reference is used):
 *   - single caller thread per handle (the reference's Solve loop is single-threaded and its static
 *     arenas are not thread-safe, include/factors_messages.hxx:3369-3370).  THREAD AFFINITY: an engine is created,
 *     used and destroyed on ONE thread.  Its streams, its block of pinned words and the staging buffer of its host
 *     copies come from (bounded) per-thread pools and go back to the pool of the thread that calls lpmp_destroy;
 *     different engines may live on different threads;
 *   - host arrays passed in are borrowed for the duration of the call; device arrays passed to
 *     lpmp_upload_model with LPMP_MEM_DEVICE are borrowed until lpmp_destroy / the next upload;
 *   - any structural change on the host side (everything that calls set_flags_dirty in the reference,
 *     include/LP_MP.h:1623) requires a new lpmp_upload_model.
 *
 * Citations are relative to /root/reference.
 */
#ifndef LPMP_ENGINE_H
#define LPMP_ENGINE_H

#include <stdint.h>
#include "lpmp_model.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lpmp_engine lpmp_engine;
typedef struct lpmp_plan lpmp_plan;

enum lpmp_status {
  LPMP_OK = 0,
  LPMP_ERR_INVALID = -1,     /* bad argument / malformed model (reference: assert / runtime_error) */
  LPMP_ERR_UNSUPPORTED = -2, /* valid in the reference but not executable on the device */
  LPMP_ERR_DEVICE = -3,      /* HIP error, or no GPU */
  LPMP_ERR_STATE = -4        /* call order (e.g. ComputePass before set_reparametrization, LP_MP.h:414,458) */
};

enum lpmp_mem { LPMP_MEM_HOST = 0, LPMP_MEM_DEVICE = 1 };

const char* lpmp_last_error(void);
const char* lpmp_version(void);
/* Always 0: there is one build of the library.  Kept for ABI compatibility. */
int lpmp_experiment_build(void);

/* ---- host-only analysis (no GPU needed) -------------------------------------------------------
 * Replaces LP::SortFactors (include/LP_MP.h:730-797), LP::get_omega (:412-460) and the weight
 * routines (:1086-1154, :1232-1449, :1489-1505); FactorContainer::get_messages
 * (include/factors_messages.hxx:3339-3365).  The cost arrays of the model are not read. */
int lpmp_plan_create(const lpmp_model* m, lpmp_plan** out);
void lpmp_plan_destroy(lpmp_plan* p);
int64_t lpmp_plan_n_factors(const lpmp_plan* p);
int64_t lpmp_plan_n_updated(const lpmp_plan* p, int direction);
int lpmp_plan_get_order(const lpmp_plan* p, int direction, int32_t* out /*[n_factors]*/);          /* forwardOrdering_ */
int lpmp_plan_get_update_order(const lpmp_plan* p, int direction, int32_t* out /*[n_updated]*/);  /* forwardUpdateOrdering_ */
int64_t lpmp_plan_omega_nnz(lpmp_plan* p, int direction);
int64_t lpmp_plan_mask_nnz(lpmp_plan* p, int direction);
int lpmp_plan_get_omega(lpmp_plan* p, int direction, int mode, int64_t* off /*[n_updated+1]*/, double* data);
int lpmp_plan_get_mask(lpmp_plan* p, int direction, int mode, int64_t* off /*[n_updated+1]*/, uint8_t* data);
int lpmp_plan_get_msg_lists(const lpmp_plan* p, int64_t* off /*[n_factors+1]*/, int64_t* entries /*[2*n_messages]: msg*2+role*/);
/* ComputeAnisotropicWeights on an arbitrary ordered factor list (include/LP_MP.h:1232-1415, incl. the
 * strict-subset rules); rows = updated members of the list.  Call with om == NULL to query sizes. */
int lpmp_plan_anisotropic_weights(const lpmp_plan* p, int64_t n, const int32_t* factors, int64_t* n_rows,
                                  int64_t* om_nnz, int64_t* mk_nnz, int64_t* om_off, double* om, int64_t* mk_off,
                                  uint8_t* mk);
/* level schedule of a built-in sweep: levels = dependent steps, launches = kernel launches */
int lpmp_plan_schedule_info(lpmp_plan* p, int direction, int mode, int64_t* n_levels, int64_t* n_launches,
                            int64_t* n_receives, int64_t* n_sends, int64_t* algorithmic_bytes);

/* updated factors of that sweep per device kernel class (LPMP_KCLASS_COUNT entries: generic, dense 4/8/16/32,
 * Potts 4/8/16/32, the run-time-dims forms of the same eight, the streaming class for up to 512 labels, the
 * lane-per-factor class for tiny factors, four classes of updated pairwise factors, four classes of unaries between
 * SHARED pairwise factors, the class of unaries between DIFF pairwise factors) */
#define LPMP_KCLASS_COUNT 28
int lpmp_plan_schedule_classes(lpmp_plan* p, int direction, int mode, int64_t* factors /*[LPMP_KCLASS_COUNT]*/);

/* Banded DIFF vectors (class diff).  The band [lo, hi] of pool entry `table` as a difference vector D of n entries:
 * every entry below lo equals D[0] and every entry above hi equals D[n - 1], compared by the bits of the doubles; lo = n and
 * hi = n - 1 for a constant vector.  banded: 1 when hi - lo + 1 <= n / 4 (such vectors are reduced in O(labels * width) per
 * receive with the same result to the bit), 0 when not, -1 (and lo 0, hi -1) when no DIFF factor references the entry. */
int lpmp_plan_n_shared_tables(const lpmp_plan* p);
int lpmp_plan_get_diff_band(const lpmp_plan* p, int table, int32_t* lo, int32_t* hi, int* banded);
/* launches of class diff in that sweep, how many of them run the banded kernel (every receive of every record of the launch
 * references a banded vector; none when LPMP_NO_DIFF_BAND was set as the plan was made), and the receives of both */
int lpmp_plan_diff_band_info(lpmp_plan* p, int direction, int mode, int64_t* diff_launches, int64_t* band_launches,
                             int64_t* diff_receives, int64_t* band_receives);
/* The same for DIFF_SHIFT factors.  The band [lo, hi] of pool entry `table` as DIFF_SHIFT factors see it: that of D
 * itself, as above, whatever the shifts; referenced: 1 when a DIFF_SHIFT factor references the entry, else 0 (and lo 0, hi -1).  A
 * receive of a d0 x d1 factor is banded when (hi - lo + 1) * 4 <= d0 + d1 - 1: the shift moves the band inside the receive's
 * d0 + d1 - 1 differences (or out of them) and never widens it, so pool values and structure decide, never a shift. */
int lpmp_plan_get_diff_shift_band(const lpmp_plan* p, int table, int32_t* lo, int32_t* hi, int* referenced);
/* launches of class diff with a DIFF_SHIFT factor in that sweep, how many of them run the shifted banded kernel (every receive of
 * every record of the launch is banded, a plain DIFF peer by its own rule; none when LPMP_NO_DIFF_BAND was set as the plan was
 * made), and the receives of both.  lpmp_plan_diff_band_info counts none of them as band launches. */
int lpmp_plan_diff_shift_band_info(lpmp_plan* p, int direction, int mode, int64_t* shift_launches, int64_t* shift_band_launches,
                                   int64_t* shift_receives, int64_t* shift_band_receives);
/* host only: new VALUES for the pool of a plan, packed as lpmp_model.sh_data (same n_shared_tables, sh_off, dims).  A NaN entry is
 * refused (LPMP_ERR_INVALID naming the table, the plan untouched), as are a NULL pointer and a plan without a pool.  The band of
 * every entry a DIFF or DIFF_SHIFT factor references is detected again (LPMP_NO_DIFF_BAND stays what it was when the plan was made), and in every
 * schedule the plan has cached each launch of class diff gets its kernel choice again by the rule above: nothing else of a schedule
 * moves and none is built.  lpmp_plan_get_diff_band / lpmp_plan_diff_band_info and their
 * DIFF_SHIFT counterparts report the new state. */
int lpmp_plan_set_shared_pool(lpmp_plan* p, const double* sh_data);

/* the same summary for an iterator-range pass (LP_MP.h:981-1005) given as factor list + weight rows + receive-mask
 * rows, without a device: what lpmp_schedule_create[_fused] would build.  Arguments as lpmp_compute_pass_custom. */
int lpmp_plan_custom_schedule_info(lpmp_plan* p, int64_t n, const int32_t* factors, const int64_t* omega_off,
                                   const double* omega, const int64_t* mask_off, const uint8_t* mask, int fuse,
                                   int64_t* n_levels, int64_t* n_launches, int64_t* n_receives, int64_t* n_sends,
                                   int64_t* algorithmic_bytes);

/* dependent step (1-based level; 0 = no active message) of every entry of the update order in that sweep (computed alone when the
 * sweep has not been planned: a multi-GPU host asks for the level structure of a global model it never runs as such) */
int lpmp_plan_get_update_levels(lpmp_plan* p, int direction, int mode, int32_t* out /*[n_updated]*/);
/* the same for a whole pass (forward then backward sweep scheduled as one sequence; back-to-back updates
 * of one factor across the two sweeps are folded into one record) */
int lpmp_plan_pass_schedule_info(lpmp_plan* p, int mode, int64_t* n_levels, int64_t* n_launches,
                                 int64_t* n_receives, int64_t* n_sends, int64_t* algorithmic_bytes);

/* chain executor: how a deep sweep (direction 0 / 1, or -1 for the fused forward+backward pass) is run —
 * persistent launches (one per kernel class), their tickets and dependencies, and the launches that stay plain;
 * all 0 when the sweep runs as ordinary launches / graph replay */
int lpmp_plan_chain_info(lpmp_plan* p, int direction, int mode, int64_t* n_chains, int64_t* n_tickets, int64_t* n_dependencies,
                         int64_t* n_plain_launches);
/* ... and how many message vectors of that sweep travel between dependent records through the chain's mailbox (tagged
 * granules polled by the receiving record instead of a completion flag followed by a fetch): rows = sends
 * that also write a mailbox row, receives = receives that poll one.  0 / 0: every hand-over goes through flags. */
int lpmp_plan_mailbox_info(lpmp_plan* p, int direction, int mode, int64_t* n_rows, int64_t* n_receives);
/* ... and, where a chain of that sweep is a LEVEL LOOP (many tiny levels of the generic or the lane-per-factor class walked by
 * one workgroup), which body its launches take.  Read-only; every pointer may be null.
 *   n_launches             launches of all level loops of the sweep (0: none)
 *   n_lane_launches        those of the lane-per-factor class; the rest run one wave per factor
 *   n_label_ops            lane-per-factor launches whose records run with one lane per OP (labeling-list records with the
 *                          factor on the left, at most 8 receives and 8 sends, no two of a kind on one peer); the other
 *                          lane-per-factor launches run one lane per factor inside the loop
 *   n_label_paired         ... of these, launches in which every record receives and then sends each of its messages
 *   n_label_staged         ... of n_label_ops, launches of at most 16 records: records, ops and match tables are staged in LDS
 *                          (with the shared send rule and without rounding; otherwise every launch reads them from memory)
 *   n_label_paired_staged  launches counted in both */
int lpmp_plan_level_loop_info(lpmp_plan* p, int direction, int mode, int64_t* n_launches, int64_t* n_lane_launches,
                              int64_t* n_label_ops, int64_t* n_label_paired, int64_t* n_label_staged, int64_t* n_label_paired_staged);

/* 1 when lpmp_compute_pass(n >= 2) joins the tail of a pass with the head of the next one for this mode (2-colour
 * orders: n passes = H, W, (K, W) x (n-1), T) — decided by an op-by-op comparison of the fused
 * schedules; 0 when consecutive passes run one after the other; negative lpmp_status on error */
int lpmp_plan_pass_rotates(lpmp_plan* p, int mode);
/* 1 when the STRUCTURE of this mode's joined passes allows the peer-minima form (the W records publish per edge
 * what the record at the other end would compute from the table, K / T read no table): exact 32-label dense class, every W
 * record sends over exactly the <= 4 edges it receives from, every receive of K / T served by exactly one W record.  The
 * engine further needs f64 tables in the packed layout and LPMP_NO_PEER_MINIMA unset.  why (n bytes; may be null): "" or the
 * first obstacle.  0 otherwise; negative lpmp_status on error */
int lpmp_plan_peer_minima(lpmp_plan* p, int mode, char* why, int n);

/* ---- variable orders and partitions (host only; csrc/graph.cpp) ---------------------------------------------------------------
 * The sweep is Gauss-Seidel over the factor ORDER, which is the caller's input (AddFactorRelation, include/LP_MP.h:698-702; the
 * topological sort of include/topological_sort.hxx:100-144): the engine runs one launch per dependent level of whatever order it
 * is given.  A grid inserted row by row has H + W - 1 levels per directional sweep; in a 2-colour order it has 2 (C3: 14.5 against
 * 5.2 ms per pass).  Another order is another, equally valid trajectory of the dual ascent — not another algorithm.
 *
 * lpmp_plan_suggest_order: rank_of_factor[f] = position of factor f in an order in which the UPDATED factors come colour by colour
 * (two of them conflict when a message joins them or both touch a common factor; component by component: 2 colours where the
 * component has no odd cycle — a grid keeps its 2 levels beside whatever else the model holds —, else a greedy Jones-Plassmann
 * colouring with counter-hash priorities from `seed`), and every other factor keeps its place relative to
 * the updated factors around it (an MRF's pairwise factor between its two unaries, a multicut triplet behind its edges).  The
 * caller turns it into relations as a chain through all factors — AddFactorRelation(by_rank[i], by_rank[i + 1]) for consecutive
 * positions: the only topological order of that chain is the suggested one, forward, and its reverse,
 * backward — and builds its LP with those instead of its own.  n_colours (may be NULL): dependent
 * levels per directional sweep to expect.  The engine prints one line to stderr when a schedule it builds has more than 64 levels
 * (LPMP_QUIET=1 silences it). */
int lpmp_plan_suggest_order(lpmp_plan* p, uint64_t seed, int32_t* rank_of_factor /*[n_factors]*/, int32_t* n_colours);
/* the same colouring for a plain pairwise graph given as an edge list (what synthetic workloads rename their variables by):
 * rank_out[v] = position of variable v in the colour-major order (colour classes in ascending colour, inside a class by index) */
int lpmp_graph_colour_major_order(int64_t n, int64_t m, const int64_t* edge_i, const int64_t* edge_j, uint64_t seed, int64_t* rank_out /*[n]*/,
                                  int32_t* n_colours_out);
/* balanced Kernighan-Lin / label-propagation refinement of a k-way partition of that graph (lp_mp_amd/multi_gpu.py
 * refine_partition, move for move): per round every variable looks at the part most of its neighbours live in; a pseudo-random half
 * of those that would cut fewer edges there move, best gains first, while the target stays within (1 + imbalance) of the mean size */
int lpmp_graph_refine_partition(int64_t n, int64_t m, const int64_t* edge_i, const int64_t* edge_j, int32_t world, int32_t rounds,
                                double imbalance, uint64_t seed, int64_t* part_inout /*[n]*/);

/* ---- device engine --------------------------------------------------------------------------- */
/* LP<FMC>::LP(cmd) (include/LP_MP.h:589-593).  device = HIP device ordinal. */
int lpmp_create(int device, lpmp_engine** out);
void lpmp_destroy(lpmp_engine* e);
/* run all work on this hipStream_t (default: a stream owned by the engine) */
int lpmp_set_stream(lpmp_engine* e, void* hip_stream);

/* add_factor / add_message / AddFactorRelation, flattened (include/LP_MP.h:239-285, :698-702), plus the
 * packed duals as serialize_dual lists them (include/factors_messages.hxx:3196-3223).
 * const_mem / dual_mem say where m->const_data / m->dual_data live.  Device buffers (LPMP_MEM_DEVICE) are borrowed,
 * not copied: whatever fills them must have completed, or be ordered on the engine's stream (lpmp_set_stream), before
 * the next engine call — the engine's own stream is non-blocking and not ordered with the null stream.
 * Size limits of the device kernels (checked when the schedules are built, LPMP_ERR_UNSUPPORTED): a factor that is
 * updated by the wave-per-factor kernels may hold at most 512 doubles of duals and its messages at most 512 entries
 * (unaries with pairwise neighbours: 512 labels; everything else the generic kernel runs: 512 doubles); factors that
 * are only peers (pairwise tables of updated unaries) are bounded by those label counts; at most 32767 active
 * receives and 32767 active sends per updated factor.
 * What an upload leaves: the weight mode is unset (lpmp_set_reparametrization comes again before a pass: LPMP_ERR_STATE otherwise), the
 * primal labels are unset, every lpmp_schedule_create id and every read-out of the previous model is dead (ids start again at 0); the
 * send rule (lpmp_set_reparametrization_type), the speculation depth, the rows-layout and table-precision requests, persistent
 * launches and the kernel-timing accumulators stay.  The previous model is released BEFORE the new one is planned: when the call
 * fails, for whatever reason (a malformed model, LPMP_ERR_UNSUPPORTED from the table precision, float tables asked for together with
 * the rows layout, a send rule the model does not run under), the engine holds NO model afterwards and every call that needs one
 * returns LPMP_ERR_STATE until an upload succeeds. */
int lpmp_upload_model(lpmp_engine* e, const lpmp_model* m, int const_mem, int dual_mem);

/* LP::set_reparametrization, LP_MP.h:330 (+ the lazy get_omega, :412-460).  Builds the weights of that mode and, for models of up
 * to 2^20 factors, the two directional schedules — a model the device kernels cannot run is refused here (LPMP_ERR_UNSUPPORTED).
 * Larger models get every schedule on first use (lpmp_compute_pass: the fused pass schedule; lpmp_compute_forward_pass / ...: the
 * directional ones; the partitioned drivers: their own iterator-range schedules), and the same refusal then. */
int lpmp_set_reparametrization(lpmp_engine* e, int mode);
/* --reparametrizationType parsed by LP::Begin (LP_MP.h:589-593, :710-722) and switched on in the hot loop (:869-887,
 * :988-1004).  All five run on the device:
 *   shared                 UpdateFactor (factors_messages.hxx:2256-2261)
 *   residual               update_factor_residual (:2270-2279, :2960-3007)
 *   partition              compute_partition_pass over the components of the put_in_same_partition graph
 *                          (lpmp_model.part_pairs; LP_MP.h:1717-1822, :1932-1963), lpmp_set_inner_iterations passes each
 *   overlapping_partition  compute_overlapping_partition_pass (:1824-1843, :1966-2051), then the plain sweeps
 *   adaptive               update_factor_adaptive (:2263-2268, :2860-2926) with the improvement op of
 *                          lpmp_msg_flags; message types without it contribute improvement 0, as in the reference's
 *                          release build, so their factors send nothing
 * LPMP_ERR_UNSUPPORTED: residual / adaptive with batch-capable message ops; adaptive when an updated factor has a
 * message it does not send through (the reference indexes past its weight row there). */
enum lpmp_reparametrization_type {
  LPMP_RTYPE_SHARED = 0, LPMP_RTYPE_RESIDUAL = 1, LPMP_RTYPE_PARTITION = 2, LPMP_RTYPE_OVERLAPPING_PARTITION = 3,
  LPMP_RTYPE_ADAPTIVE = 4
};
int lpmp_set_reparametrization_type(lpmp_engine* e, int rtype);
int lpmp_set_inner_iterations(lpmp_engine* e, int n);       /* --innerIteration, default 5 (LP_MP.h:590) */
/* LP::construct_factor_partition (LP_MP.h:1717-1822): number of partitions; with off != NULL also their factor lists
 * (updated factors only, CSR: off[n_partitions + 1], factors[n_updated]) */
int lpmp_plan_get_partitions(lpmp_plan* p, int64_t* n_partitions, int64_t* off, int32_t* factors);
int lpmp_compute_pass(lpmp_engine* e, int n_passes);        /* LP::ComputePass, LP_MP.h:869-887 ('shared') */
/* optional: build ahead of time what lpmp_compute_pass(e, n_passes) needs that depends on n_passes (the ticket order of
 * n joined passes for the chain executor), e.g. outside of a timed region */
int lpmp_prepare_passes(lpmp_engine* e, int n_passes);
/* ---- passes that run ahead of the caller --------------------------------------------------------------------------
 * The reference's Solver asks for ONE pass per iteration and, by default, for the bound after each (Solver::Iterate /
 * PostIterate, include/solver.hxx:273-284, --lowerBoundComputationInterval 1), while the device is fastest when
 * consecutive passes are one persistent launch (lpmp_compute_pass(e, n): 5.1 against 6.6 ms per pass on C3).  With
 * max_passes_ahead >= 2, lpmp_compute_pass(e, 1) may launch up to that many passes at once (after a snapshot of the
 * duals); the next calls of lpmp_compute_pass(e, 1) only advance a cursor, and lpmp_lower_bound returns the bound after
 * the pass the caller is AT — the launch leaves one row of per-factor bounds per pass.  Every other call first settles:
 * if the caller stopped inside a batch, the duals go back to the snapshot and exactly the passes asked for are run again
 * (n joined passes equal n single ones bit for bit), so results never differ from max_passes_ahead = 0; only time does.
 * The look-ahead adapts to the caller: it doubles while single passes keep coming and restarts at the length of the
 * previous run (MpRoundingSolver: four plain passes between two rounding iterations).  Needs a pass whose consecutive
 * passes join (lpmp_plan_pass_rotates) on an HBM-sized model, send rule `shared`; otherwise every call is executed as it
 * comes.  Default 0 (off; LPMP_SPECULATION=<n> in the environment sets it for engines created afterwards); the solver
 * adapters (lpmp_offload.hxx, LP_gpu.hxx, lp.py) switch it on.  Callers that read a BORROWED dual buffer directly
 * (lpmp_device_duals, LPMP_MEM_DEVICE) call lpmp_synchronize first: it settles.  At most 32. */
int lpmp_set_speculation(lpmp_engine* e, int max_passes_ahead);
int lpmp_speculation_stats(lpmp_engine* e, int64_t* batches, int64_t* passes_launched, int64_t* passes_used, int64_t* rollbacks);
/* device bytes held by the cached ticket lists of joined-pass launches (bounded: LPMP_CHAIN_CACHE_MB, default 2048) */
int64_t lpmp_chain_cache_bytes(const lpmp_engine* e);
int lpmp_compute_forward_pass(lpmp_engine* e);              /* LP::ComputeForwardPass, LP_MP.h:889-900 */
int lpmp_compute_backward_pass(lpmp_engine* e);             /* LP::ComputeBackwardPass, LP_MP.h:902-911 */
/* LP::ComputePass(factorIt, factorItEnd, omegaIt, receive_it), LP_MP.h:981-1005: any factor list with
 * any weights / masks (one row per listed factor). */
int lpmp_compute_pass_custom(lpmp_engine* e, int64_t n, const int32_t* factors, const int64_t* om_off,
                             const double* om, const int64_t* mk_off, const uint8_t* mk);
/* The same, prepared once and replayed: the partition sweeps of the multi-GPU driver are iterator-range
 * passes (main sweep without ghost factors, boundary receive, boundary send) that run every iteration.
 * Precedent in the reference: compute_partition_pass keeps per-partition omega / mask arrays
 * (include/LP_MP.h:1846-1963). */
int lpmp_schedule_create(lpmp_engine* e, int64_t n, const int32_t* factors, const int64_t* om_off, const double* om,
                         const int64_t* mk_off, const uint8_t* mk, int* id_out);
/* as lpmp_schedule_create for a list that concatenates several sweeps (e.g. forward then backward update lists):
 * with fuse != 0 back-to-back updates of one factor are folded into one record (same results) */
int lpmp_schedule_create_fused(lpmp_engine* e, int64_t n, const int32_t* factors, const int64_t* om_off,
                               const double* om, const int64_t* mk_off, const uint8_t* mk, int fuse, int* id_out);
/* lpmp_schedule_run / _info / _destroy with an id that was never returned, that was destroyed, or that belongs to a model replaced
 * since by lpmp_upload_model (before a new schedule takes the number): LPMP_ERR_INVALID ("unknown schedule id"), nothing runs.  A run
 * settles passes that ran ahead, like every pass; the ids stay valid across lpmp_upload_costs, lpmp_set_vectors,
 * lpmp_upload_shared_pool, lpmp_set_constants, lpmp_move_windows, lpmp_zero_pairwise_duals and lpmp_upload_duals and run on the costs
 * of the moment. */
int lpmp_schedule_run(lpmp_engine* e, int id);
int lpmp_schedule_info(lpmp_engine* e, int id, int64_t* n_levels, int64_t* n_launches, int64_t* n_receives,
                       int64_t* n_sends, int64_t* algorithmic_bytes);
int lpmp_schedule_destroy(lpmp_engine* e, int id);
int lpmp_lower_bound(lpmp_engine* e, double* out);          /* LP::LowerBound, LP_MP.h:1507-1518 */
int lpmp_factor_lower_bounds(lpmp_engine* e, double* out /*[n_factors], host*/); /* FactorTypeAdapter::LowerBound */
/* The two scalars into the caller's DEVICE memory: exactly one double is written, asynchronously on the engine's stream.  There is no
 * stream synchronisation and no device-to-host copy on either path, so a stopping rule, a loss or a log that lives in device code
 * never stalls the stream; an aborted persistent launch is reported by the next call that synchronises, as for device read-outs.
 * The value is bit for bit what the host call returns on the same state: the model constant plus the partial sums of the two-stage
 * sum, added in ascending order by one thread, no contraction.
 *   lpmp_lower_bound_dev      the stale count never reaches the host: when the engine knows that every tracked bound is stale (an
 *     upload, lpmp_upload_costs, lpmp_invalidate_lower_bounds, ...) every factor is recomputed; otherwise the stale entries are
 *     collected and recomputed by a launch of fixed size that reads their number on the device — however many there are (the host
 *     call recomputes everything above an eighth; the per-factor values are the same).  Inside an open batch of passes that ran
 *     ahead it reads the row of the pass the caller is at, like lpmp_lower_bound, and does not settle.
 *     lpmp_lower_bound_recomputed keeps the value of the last HOST call.  LPMP_ERR_STATE while the constants are unspecified.
 *   lpmp_evaluate_primal_dev  settles first, as the host call; +inf when a side disagrees or a slot is unset (the last kernel reads
 *     the consistency flag on the device).  LPMP_ERR_UNSUPPORTED on a model the rounding code refuses, as the host call;
 *     LPMP_ERR_STATE before an upload and while the constants are unspecified.
 * LPMP_ERR_INVALID for a null pointer.  Rows layout and both f32 table modes work unchanged. */
int lpmp_lower_bound_dev(lpmp_engine* e, double* dst_dev);
int lpmp_evaluate_primal_dev(lpmp_engine* e, double* dst_dev);
/* The sweep kernels keep a per-factor lower bound current as a by-product, so lpmp_lower_bound after
 * a pass is a sum over an array.  Call this after changing duals behind the engine's back (writes through
 * lpmp_device_duals or a borrowed dual buffer): the next lpmp_lower_bound recomputes every factor.
 * Order of a direct access to a BORROWED dual buffer: lpmp_synchronize (or lpmp_device_duals) FIRST — it settles passes that ran
 * ahead and, with the rows layout, writes the dense pairwise vectors out to the packed array —, then read / write, then this call.
 * Without the first step, under the rows layout the pairwise vectors read are stale and what was written into them is replaced
 * by the rows' contents here (vector factors live in the packed array only and are not affected).  The lpmp_boundary_* and
 * lpmp_halo_* calls need none of this: they address the rows themselves. */
int lpmp_invalidate_lower_bounds(lpmp_engine* e);
/* How many per-factor bounds the last lpmp_lower_bound / lpmp_factor_lower_bounds had to recompute from the duals (the sweep
 * kernels keep the others current: DESIGN.md 5); the number of factors when it recomputed everything, -1 before the first. */
int64_t lpmp_lower_bound_recomputed(const lpmp_engine* e);
int lpmp_synchronize(lpmp_engine* e);
/* Calls that move no value — no dual, no bound beyond the rounding of a recomputed sum, no label, no schedule: lpmp_set_speculation,
 * lpmp_set_persistent_launches, lpmp_enable_kernel_timing, lpmp_invalidate_lower_bounds and lpmp_synchronize settle passes that ran
 * ahead; lpmp_prepare_passes, lpmp_reset_kernel_timing and the getters (lpmp_speculation_stats, lpmp_chain_cache_bytes,
 * lpmp_get_kernel_timing, ...) do not.  lpmp_lower_bound inside an open batch reads that pass's row and does not settle either. */
/* diagnostic: 1 when the uploaded model is streamed with non-temporal loads / stores (tables + duals above 1 GiB, i.e.
 * far larger than L2 + Infinity Cache; LPMP_NT=0/1 in the environment overrides), else 0; -1 without a model */
int lpmp_streaming_access(const lpmp_engine* e);

/* ---- primal rounding inside the sweep -----------------------------------------------------------
 * UpdateFactorPrimal (include/factors_messages.hxx:2332-2373): the same receives and (always 'shared') sends; in
 * between, every factor of a COMPUTE_PRIMAL_SOLUTION type (lpmp_model.ftype_computes_primal) takes the first
 * minimiser of its reparametrised costs as its label unless it already holds one of this time stamp
 * (conditionally_init_primal :3302-3309, MaximizePotentialAndComputePrimal :2382-2389), and the label is copied into
 * the adjacent pairwise factors (propagate_primal_through_messages :2391-2403, :1313-1328).  Built for unary /
 * pairwise models: COMPUTE_PRIMAL vector factors on the left of unary-pairwise messages (LP_MP-MRF's FMC_SRMP), and
 * COMPUTE_PRIMAL pairwise factors (`right` / `full` schedules, MPLP-style): an updated one fills its free sides with
 * the first minimiser in row-major order given the labels its unaries hold and labels those unaries
 * (ComputeLeftFromRightPrimal :1330-1344, then the recursion into their other pairwise factors).  Other message
 * kinds, or two unaries on one side of a pairwise factor, return LPMP_ERR_UNSUPPORTED.  Time stamps as in the
 * reference: 2*iteration+1 / +2. */
int lpmp_compute_forward_pass_and_primal(lpmp_engine* e, uint64_t iteration);   /* LP::ComputeForwardPassAndPrimal, LP_MP.h:914-923 */
int lpmp_compute_backward_pass_and_primal(lpmp_engine* e, uint64_t iteration);  /* LP::ComputeBackwardPassAndPrimal, LP_MP.h:925-934 */
int lpmp_compute_pass_and_primal(lpmp_engine* e, uint64_t iteration);           /* LP::ComputePassAndPrimal, LP_MP.h:936-940 */
int lpmp_check_primal_consistency(lpmp_engine* e, int* consistent);             /* LP::CheckPrimalConsistency, LP_MP.h:1067-1082 */
int lpmp_evaluate_primal(lpmp_engine* e, double* cost);                         /* LP::EvaluatePrimal, LP_MP.h:1521-1536 (+inf when inconsistent / unset) */
/* the factors' primal_ members, what serialize_primal lists: [2*n_factors] int32, vector factor (label, 0), pairwise
 * factor (x0, x1); an unset entry holds the dimension (init_primal) */
int lpmp_download_primal(lpmp_engine* e, int32_t* host_out);
int lpmp_upload_primal(lpmp_engine* e, const int32_t* host_in);

/* ---- labels from the duals: conditional rounding -------------------------------------------------------------------
 * The extraction of TRW-S / SRMP: walk the unaries in the sweep order and give each the minimiser of its reparametrised cost
 * CONDITIONED on the labels its already-visited neighbours got.  Reads the duals, writes only the primal array that
 * lpmp_download_primal / lpmp_evaluate_primal / lpmp_check_primal_consistency read.  No counterpart in the reference.
 *
 * Supported models: every message is LPMP_M_UNARY_PAIRWISE, and every pairwise factor (DENSE in any table precision, POTTS,
 * SHARED, DIFF) has exactly one such message on each side, from two DIFFERENT unaries.  Anything else — a message of another
 * kind, a side without a unary or with two, one unary on both sides — is LPMP_ERR_UNSUPPORTED naming the lowest offending factor.
 * Decoded unaries: every VECTOR factor.  Decode order pi: lpmp_plan_get_order(plan, direction) restricted to them.
 *
 * Per unary u with d0 labels:
 *   c[x] = theta_u[x]                                            (the current dual)
 *   for every message k of u, in ascending MESSAGE INDEX, whose pairwise factor p has its other unary v LABELLED:
 *       s = side of u in p;  t[x] = cost_p(x, x_v) if s == 0 else cost_p(x_v, x)
 *       c[x] = c[x] + (t[x] + m_s[x])                            (m_s: p's dual vector of side s; the inner sum first)
 *   x_u = the smallest x with c[x] == min_x c[x]
 * cost_p is the pairwise cost of lpmp_model.h (DENSE: the table entry, floats widened; POTTS: a == b ? 0.0 : diff; SHARED / DIFF:
 * ONE multiply scale * entry).  All arithmetic is IEEE double in this order, no contraction.  +inf entries are allowed (all +inf:
 * label 0); NaN is outside the contract.
 *   initial sweep        "labelled" = earlier in pi
 *   refine_sweeps >= 0   further sweeps over pi in which EVERY neighbour counts: those earlier in pi with this sweep's label, the
 *                        others with the previous sweep's.  With all neighbours theta_u + sum m_s is the original unary, so a
 *                        refinement sweep is ICM on the original energy: the primal cost never rises over these sweeps.
 * Afterwards both slots of every pairwise factor take the labels of its unaries.
 * Direction: decode AGAINST the direction of the last sweep (after lpmp_compute_pass, which ends with a backward sweep: LPMP_FORWARD),
 * as TRW-S does — on chains that is the exact optimum, the other direction is not.
 *
 * Settles passes that ran ahead first; asynchronous on the engine's stream like a pass.  Duals, tracked bounds, weights, schedules
 * and kernel timing do not move; a later ..._pass_and_primal behaves as after lpmp_upload_primal.  The primal array is allocated on
 * first use whatever ftype_computes_primal says.  The device tables of a direction are structure: built on the first call (one
 * launch per level and label-count class: the levels of lpmp_plan_get_decode_levels), counted by lpmp_schedules_built, kept across
 * lpmp_upload_costs / lpmp_upload_shared_pool / lpmp_set_constants / lpmp_set_vectors, dropped by lpmp_upload_model.
 * LPMP_ERR_STATE before lpmp_upload_model; LPMP_ERR_INVALID for a direction other than 0 / 1 or refine_sweeps < 0. */
int lpmp_decode_primal(lpmp_engine* e, int direction, int refine_sweeps);
/* host only: the structure of that decode.  n_unaries decoded unaries, n_levels dependent levels (level(u) = 1 + the highest level of
 * a neighbour earlier in pi, 1 without one: neighbours never share a level, so a level is one launch), n_links unary-pairwise links;
 * any pointer may be NULL.  lpmp_plan_get_decode_levels: factor_out[i] = i-th unary of pi, level_out[i] its level (n_unaries each).
 * LPMP_ERR_UNSUPPORTED with the refusal above. */
int lpmp_plan_decode_info(lpmp_plan* p, int direction, int64_t* n_unaries, int64_t* n_levels, int64_t* n_links);
int lpmp_plan_get_decode_levels(lpmp_plan* p, int direction, int32_t* factor_out, int32_t* level_out);

/* ---- prepared read-outs: labels, unaries and beliefs of listed VECTOR factors into the caller's array ---------------
 * The output twin of lpmp_set_vectors.  A read-out is a prepared list of VECTOR factors, like an lpmp_schedule_create id or an
 * lpmp_halo: its record tables are uploaded once, a call plans and uploads nothing.
 * lpmp_readout_create: `factors` is a host array of n VECTOR factor indices in the caller's order (a factor may be listed twice: reads
 * are idempotent, both rows get the same content); factors == NULL: every VECTOR factor in ascending index, n is ignored.  n == 0
 * makes an empty read-out whose calls are no-ops after their checks.  LPMP_ERR_STATE before lpmp_upload_model; LPMP_ERR_INVALID,
 * naming the offender, for an index out of range or a non-VECTOR factor.  The object is structure: it stays valid across
 * lpmp_upload_costs, lpmp_set_vectors, lpmp_upload_shared_pool, lpmp_set_constants, lpmp_zero_pairwise_duals, passes and decodes;
 * after the next lpmp_upload_model every call on it returns LPMP_ERR_STATE (destroying it stays legal); lpmp_destroy does not free
 * it.  lpmp_schedules_built does not move at create: the link tables behind the beliefs are built on the first lpmp_readout_beliefs
 * of a read-out and counted once then.
 *
 * Common to the three calls: they settle passes that ran ahead first (the state read is that of the pass the caller is at); duals,
 * tracked bounds, the primal array, weights, schedules, kernel timing and speculation depth do not move; nothing is written but dst.
 * dst_mem == LPMP_MEM_DEVICE: asynchronous on the engine's stream like a pass, no host synchronisation (so an aborted persistent
 * launch is reported by the next call that synchronises, as after lpmp_decode_primal, not here).  LPMP_MEM_HOST: through a
 * buffer of the engine, the call returns after the copy.  Row i starts at dst + i * dst_stride; entries of a row beyond the
 * factor's dim0 are not written; dst_stride < lpmp_readout_max_labels is LPMP_ERR_INVALID.
 *   labels   dst[i] = the label slot of factor factors[i] exactly as lpmp_download_primal reports it (an unset entry holds the
 *            dimension).  The primal array is allocated on first use, as in lpmp_decode_primal.  Every model — on one the rounding
 *            code refuses (messages other than unary-pairwise) no call can set a label and every entry is the dimension.
 *   vectors  row i = the current theta of the factor.  Every model, every layout.
 *   beliefs  per-label min-marginal estimates.  A listed unary u with d0 labels gets
 *              b[x] = theta_u[x]
 *              for every message k of u IN THE ORDER OF u's MESSAGE LIST (lpmp_plan_get_msg_lists: the order in which a sweep
 *              receives), p its pairwise factor and s the side of u in p:
 *                  q[x] = min_y (cost_p(x, y) + m_o[y]) for s == 0, cost_p(y, x) for s == 1       (m_o: p's vector of the other side)
 *                  b[x] = b[x] + (m_s[x] + q[x])
 *            cost_p as in lpmp_decode_primal (ONE multiply for SHARED / DIFF, floats widened under the f32 table modes); all
 *            arithmetic IEEE double in this order, no contraction.  +inf entries are allowed, NaN is outside the contract, which
 *            zero a minimum over -0.0 and +0.0 returns is unspecified.  This is bit for bit the theta_u the receive phase of a sweep
 *            would produce if u received over all its messages and sent nothing.  NOT the ascending-message-index order of the
 *            decode.  Supported per listed factor: every message of u is LPMP_M_UNARY_PAIRWISE with u as its left factor (the peer
 *            DENSE in any table precision, POTTS, SHARED or DIFF); a unary without messages gets theta.  Otherwise
 *            LPMP_ERR_UNSUPPORTED naming the lowest such listed factor (checked at create and stored; labels and vectors stay
 *            usable).  LPMP_ERR_STATE while the constants are unspecified (a refused lpmp_upload_costs). */
typedef struct lpmp_readout lpmp_readout;
int lpmp_readout_create(lpmp_engine* e, int64_t n, const int32_t* factors, lpmp_readout** out);
void lpmp_readout_destroy(lpmp_readout* r);
int64_t lpmp_readout_n(const lpmp_readout* r);          /* rows */
int32_t lpmp_readout_max_labels(const lpmp_readout* r); /* longest listed vector */
int lpmp_readout_labels(lpmp_engine* e, lpmp_readout* r, int32_t* dst, int dst_mem);
/* The input twin of lpmp_readout_labels: src[i] (int32, host or device: src_mem) becomes the label of factors[i].  0 ... d0 - 1 is a
 * label, d0 (the dimension) means unset, exactly what lpmp_readout_labels reports: what one call wrote the other reads back.
 *   host source    a value outside [0, d0] is LPMP_ERR_INVALID naming the entry, with nothing written; the call returns after its copy
 *   device source  a value outside [0, d0 - 1] is stored as unset where it is read (the saturated device delta of lpmp_move_windows is
 *                  the precedent): no bit pattern is copied into the primal array unchecked.  Asynchronous on the engine's stream, no
 *                  host synchronisation
 * A read-out that lists a factor twice is refused by THIS call (LPMP_ERR_INVALID naming the factor; decided at lpmp_readout_create and
 * stored): two rows would write one slot.  labels / vectors / beliefs stay usable on it.
 * The primal array is made on first use exactly as lpmp_readout_labels makes it, the array of unset labels of a model the rounding
 * code refuses included: there only the unaries' labels are written, as path moves do.  Otherwise both slots of every pairwise
 * factor take the labels of its unaries, as after a decode: a label that is SET is copied, so a unary given as unset leaves its
 * pairwise slots as they were (lpmp_evaluate_primal is +inf either way).  Labels of unlisted unaries stay.  A later
 * ..._pass_and_primal behaves as after lpmp_upload_primal.  Settles passes that ran ahead; moves no dual, bound, weight, schedule or
 * timing state; lpmp_schedules_built does not move.  This is how lpmp_path_moves / lpmp_forest_moves — block coordinate descent FROM
 * the labels the primal array holds — start from a labelling that lives on the device (the previous frame, the coarse level, a
 * network's arg-max).  LPMP_ERR_STATE for a read-out of a model replaced since; LPMP_ERR_INVALID for a null source (n > 0) or a bad
 * src_mem; n == 0 is a no-op after the checks. */
int lpmp_readout_set_labels(lpmp_engine* e, lpmp_readout* r, const int32_t* src, int src_mem);
int lpmp_readout_vectors(lpmp_engine* e, lpmp_readout* r, double* dst, int64_t dst_stride, int dst_mem);
int lpmp_readout_beliefs(lpmp_engine* e, lpmp_readout* r, double* dst, int64_t dst_stride, int dst_mem);

/* ---- path moves: exact relabelling of whole paths given all other labels ------------------------------------------
 * Block coordinate descent on the labels: take a path of the graph (a row or a column of a grid), keep every other label, and give
 * the path the labels that minimise the energy over it, by dynamic programming.  Reads the duals, the constants and the primal
 * array, writes only the primal array that lpmp_download_primal / lpmp_evaluate_primal / lpmp_readout_labels read.  No counterpart
 * in the reference.
 *
 * A path set is a prepared object like an lpmp_readout or an lpmp_window_set.  It holds n_groups groups; group g is the paths
 * [group_off[g], group_off[g+1]); path j is the entries [path_off[j], path_off[j+1]) of `unaries`: k >= 1 distinct VECTOR factors
 * u_0 ... u_{k-1} of the uploaded model.  Consecutive members are joined by exactly one pairwise factor e_i between u_i and
 * u_{i+1}, the path edge; the engine finds it.  A unary may appear in several groups (rows and columns), never twice in one.
 *
 * lpmp_path_moves runs the groups in the given order, `rounds` times.  The paths of a group are independent (no pairwise factor
 * joins two of them) and run concurrently.  For one path, with x_v the label unary v holds in the primal array:
 *   node cost   n_i[x] = theta_{u_i}[x]                                  (the current dual)
 *               for every message of u_i, in ascending MESSAGE INDEX as in lpmp_decode_primal; p its pairwise factor, s the side
 *               of u_i in p, v the unary on the other side:
 *                   p is e_{i-1} or e_i:   n_i[x] = n_i[x] + m_s[x]
 *                   otherwise:             n_i[x] = n_i[x] + (t[x] + m_s[x]),  t[x] = cost_p(x, x_v) if s == 0 else cost_p(x_v, x)
 *               (m_s: p's dual vector of side s; the inner sum first).  x_v is clamped into [0, d_v - 1] where it is read, as the
 *               decode kernel does: a neighbour without a label is outside the energy guarantee, but no bit pattern reads
 *               outside a table.
 *   forward     f_0 = n_0;  for i >= 1:  g_i[y] = min_x (f_{i-1}[x] + c_i(x, y)),  back_i[y] = the smallest minimising x,
 *               f_i[y] = g_i[y] + n_i[y],  with c_i(x, y) = cost_{e_{i-1}}(x, y) when u_{i-1} is on side 0 of the edge and
 *               cost_{e_{i-1}}(y, x) otherwise
 *   backwards   x_{k-1} = the smallest minimiser of f_{k-1};  x_{i-1} = back_i[x_i].  The new labels go to the primal array.
 * cost_p is the pairwise cost of lpmp_model.h as in lpmp_decode_primal (ONE multiply for SHARED / DIFF / DIFF_SHIFT, floats widened
 * under the f32 table modes).  All arithmetic is IEEE double in this order, no contraction.  +inf entries are allowed (an all +inf
 * column: back-pointer 0; an all +inf f_{k-1}: label 0); NaN is outside the contract.  After the last group of the last round both
 * slots of every pairwise factor take the labels of its unaries, as after a decode.
 * The sum of n_i[x_i] over the path plus the sum of c_{i+1}(x_i, x_{i+1}) is every term of the energy that depends on the path's
 * labels, written with theta_u + sum m_s as the unaries (the original unaries up to rounding): on a complete labelling
 * the primal cost never rises over a path, a group or a round.  A path of one member is one step of the decode's refinement sweep;
 * a path that is the whole of a chain model gives the optimum whatever the duals are.
 *
 * lpmp_path_set_create: LPMP_ERR_STATE before lpmp_upload_model.  Checked in this order, the first failure reported:
 *   LPMP_ERR_INVALID, naming the entry: offsets that are not monotone (group_off[0] and path_off[0] are 0; a path has at least one
 *     member); an index out of range or a non-VECTOR factor; a unary that appears twice in one group, in one path or in two;
 *   LPMP_ERR_UNSUPPORTED, naming the lowest offending listed unary u: a message of u that is not LPMP_M_UNARY_PAIRWISE with u as
 *     its left factor; an adjacent pairwise factor that does not have exactly one unary on each side, from two different unaries;
 *     more than 512 labels;
 *   LPMP_ERR_INVALID, naming the entries: consecutive members joined by no pairwise factor, or by more than one; a pairwise factor
 *     that joins two non-consecutive members of one path (a closed ring included), or members of two paths of one group.
 * Unlisted parts of the model may be anything.  On a model the rounding code refuses (a message of another kind off the paths) the
 * primal array is the array of unset labels lpmp_readout_labels makes: the paths' unaries get labels, no pairwise slot is written.
 * At create the record / link / edge tables and the back-pointer scratch are built and uploaded — the scratch holds the
 * back-pointers of the largest group, one byte per entry where the previous member has at most 256 labels, two above
 * (lpmp_path_set_scratch_bytes) — and lpmp_schedules_built counts the create ONCE; a move plans and uploads nothing.  n_groups == 0
 * or groups without paths: a set whose moves are no-ops after their checks.
 * The set is structure: it stays valid across lpmp_upload_costs, lpmp_set_vectors, lpmp_upload_shared_pool, lpmp_set_constants,
 * lpmp_move_windows, lpmp_zero_pairwise_duals, passes and decodes; after the next lpmp_upload_model every move on it returns
 * LPMP_ERR_STATE (destroying it stays legal); lpmp_destroy does not free it.
 *
 * lpmp_path_moves settles passes that ran ahead first, needs specified constants (LPMP_ERR_STATE while they are not, as the
 * decode), allocates the primal array on first use, and is asynchronous on the engine's stream: one plain launch per group, form
 * (a wave per path while no member has more than 64 labels, a workgroup per path above) and round.  Duals, tracked bounds,
 * weights, schedules, kernel timing and speculation depth do not move.  rounds < 0: LPMP_ERR_INVALID; rounds == 0: a no-op after
 * the checks.  Works under the rows layout and both f32 table modes. */
typedef struct lpmp_path_set lpmp_path_set;
int lpmp_path_set_create(lpmp_engine* e, int64_t n_groups, const int64_t* group_off /* [n_groups + 1], in paths */,
                         const int64_t* path_off /* [n_paths + 1], in entries */, const int32_t* unaries, lpmp_path_set** out);
void lpmp_path_set_destroy(lpmp_path_set* ps);
int64_t lpmp_path_set_n_groups(const lpmp_path_set* ps);
int64_t lpmp_path_set_n_paths(const lpmp_path_set* ps);
int64_t lpmp_path_set_longest(const lpmp_path_set* ps);        /* members of the longest path */
int64_t lpmp_path_set_scratch_bytes(const lpmp_path_set* ps);
int lpmp_path_moves(lpmp_engine* e, lpmp_path_set* ps, int rounds);
/* host only: the checks of lpmp_path_set_create on a plan, and the counts: paths, path edges (sum of k - 1), links of listed unaries
 * that are no path edge (one cost line each per move; a unary listed in two groups counts in both).  Any pointer may be NULL; on
 * failure `why` (why_n bytes) receives the message of lpmp_last_error. */
int lpmp_plan_path_info(lpmp_plan* p, int64_t n_groups, const int64_t* group_off, const int64_t* path_off, const int32_t* unaries,
                        int64_t* n_paths, int64_t* n_path_edges, int64_t* n_off_path_links, char* why, int why_n);

/* ---- forest moves: exact relabelling of induced forests given all other labels ------------------------------------
 * The path move for any graph: a path is a tree, and the dynamic programme that is exact on a path is exact on any set of unaries
 * whose induced subgraph is a forest — leaf-to-root min-plus, then root-to-leaf back-tracking.  Reads the duals, the constants and
 * the primal array, writes only the primal array.  No counterpart in the reference.
 *
 * A forest set is a prepared object like an lpmp_path_set.  It holds n_groups groups; group g is the entries
 * [group_off[g], group_off[g+1]) of two parallel arrays: unaries[i] is a VECTOR factor of the uploaded model, parent[i] the FACTOR
 * INDEX of the parent of unaries[i], or -1 for a root.  The parent is listed in the same group.  A unary may be in several groups,
 * never twice in one.  A child and its parent are joined by exactly one pairwise factor, the tree edge; the engine finds it.
 *
 * lpmp_forest_moves runs the groups in the given order, `rounds` times.  The trees of a group are independent and run concurrently.
 * For one group, with x_v the label unary v holds in the primal array when the group starts:
 *   children    of v: the members whose parent is v, in ascending MESSAGE INDEX of v's message into the tree edge
 *   node cost   exactly as in lpmp_path_moves:  n_v[x] = theta_v[x];  then every message of v in ascending message index, p its
 *               pairwise factor, s the side of v, w the other unary:
 *                   p is a tree edge (to the parent or to a child):   n_v[x] = n_v[x] + m_s[x]
 *                   otherwise:             n_v[x] = n_v[x] + (t[x] + m_s[x]),  t[x] = cost_p(x, x_w) if s == 0 else cost_p(x_w, x)
 *               x_w is clamped into [0, d_w - 1] where it is read
 *   up          children before parents:  f_v[x] = n_v[x];  then for every child c in the order above  f_v[x] = f_v[x] + g_c[x].
 *               A non-root v with parent q and tree edge e:  g_v[y] = min_x (f_v[x] + c_v(x, y)),  back_v[y] = the smallest
 *               minimising x (ascending x, strict <),  c_v(x, y) = cost_e(x, y) when v is on side 0 of e and cost_e(y, x) otherwise
 *   down        x_r = the smallest minimiser of f_r for a root;  x_v = back_v[x_q] otherwise.  The new labels go to the primal array.
 * cost_p, the arithmetic (IEEE double in this order, no contraction), +inf (an all +inf column: back-pointer 0; an all +inf f_r:
 * label 0), NaN (outside the contract) and the propagation into the pairwise slots after the last group of the last round are those
 * of lpmp_path_moves, and so is the treatment of a model the rounding code refuses.  Consequences:
 *   paths        IEEE addition is commutative (n + g has the bits of g + n): a group whose trees are the paths u_0 ... u_{k-1} with
 *                parent[u_i] = u_{i+1} gives bit for bit the labels of lpmp_path_moves on those paths
 *   single nodes a tree of one node is one step of the decode's refinement sweep
 *   energy       sum_v n_v[x_v] + sum over the tree edges c_v(x_v, x_q) is every term of the energy that depends on the group's
 *                labels (no pairwise factor joins two trees): on a complete labelling the primal cost never rises over a group
 *   tree models  a group that is the whole of a tree-structured model gives the optimum whatever the duals are
 *
 * lpmp_forest_set_create: LPMP_ERR_STATE before lpmp_upload_model.  Checked in this order, the first failure reported:
 *   LPMP_ERR_INVALID, naming the entry: offsets that are not monotone, or group_off[0] != 0; an index out of range or a non-VECTOR
 *     factor; a unary twice in one group; a parent that is neither -1 nor a member of the same group, or is the entry itself;
 *     parent pointers that close a cycle (the lowest entry on one is named);
 *   LPMP_ERR_UNSUPPORTED, naming the lowest offending listed unary: the refusals of lpmp_path_set_create (a message that is not
 *     LPMP_M_UNARY_PAIRWISE with the unary on the left; an adjacent pairwise factor without exactly one unary on each side from two
 *     different unaries; more than 512 labels);
 *   LPMP_ERR_INVALID, naming the entries: a child and its parent joined by no pairwise factor, or by more than one; a pairwise
 *     factor that joins two members of one group that are not child and parent (a chord, an edge between two trees): the members
 *     of a group must induce a forest.
 * At create the node / link / child tables, the launch lists (per group: its nodes by height and form, then by depth) and the
 * scratch are built and uploaded; lpmp_schedules_built counts the create ONCE; a move plans and uploads nothing.  The scratch holds,
 * per non-root node of the largest group, d_parent doubles (g_v) and d_parent back-pointers, one byte each while d_v <= 256, two
 * above (lpmp_forest_set_scratch_bytes).  n_groups == 0 or empty groups: a set whose moves are no-ops after their checks.
 * The set is structure: it stays valid across lpmp_upload_costs, lpmp_set_vectors, lpmp_upload_shared_pool, lpmp_set_constants,
 * lpmp_move_windows, lpmp_zero_pairwise_duals, passes and decodes; after the next lpmp_upload_model every move on it returns
 * LPMP_ERR_STATE (destroying it stays legal); lpmp_destroy does not free it.
 *
 * lpmp_forest_moves settles passes that ran ahead first, needs specified constants (LPMP_ERR_STATE while they are not, as the
 * decode), allocates the primal array on first use, and is asynchronous on the engine's stream: per group and round one plain
 * launch per height level and form (a wave per node while neither the node nor its parent has more than 64 labels, a workgroup
 * per node above) and one per depth level >= 1.  Duals, tracked bounds, weights, schedules, kernel timing and speculation depth do
 * not move.  rounds < 0: LPMP_ERR_INVALID; rounds == 0: a no-op after the checks.  Works under the rows layout and both f32 table
 * modes. */
typedef struct lpmp_forest_set lpmp_forest_set;
int lpmp_forest_set_create(lpmp_engine* e, int64_t n_groups, const int64_t* group_off /* [n_groups + 1], in entries */,
                           const int32_t* unaries, const int32_t* parent, lpmp_forest_set** out);
void lpmp_forest_set_destroy(lpmp_forest_set* fs);
int64_t lpmp_forest_set_n_groups(const lpmp_forest_set* fs);
int64_t lpmp_forest_set_n_trees(const lpmp_forest_set* fs);
int64_t lpmp_forest_set_max_height(const lpmp_forest_set* fs);   /* edges on the longest leaf-to-root walk: dependent up launches - 1 */
int64_t lpmp_forest_set_scratch_bytes(const lpmp_forest_set* fs);
int lpmp_forest_moves(lpmp_engine* e, lpmp_forest_set* fs, int rounds);
/* host only: the checks of lpmp_forest_set_create on a plan, and the counts: trees (roots), tree edges (non-roots), links of listed
 * unaries that are no tree edge (one cost line each per move; a unary listed in two groups counts in both), the highest height (0
 * for sets of single nodes and for empty sets).  Any pointer may be NULL; on failure `why` receives the message of lpmp_last_error. */
int lpmp_plan_forest_info(lpmp_plan* p, int64_t n_groups, const int64_t* group_off, const int32_t* unaries, const int32_t* parent,
                          int64_t* n_trees, int64_t* n_tree_edges, int64_t* n_off_tree_links, int64_t* max_height, char* why, int why_n);
/* host only: a cover of any model by forest groups, in the arrays of lpmp_forest_set_create.  Call once with NULL arrays for
 * *n_groups and *n_entries, then with group_off [n_groups + 1], unaries and parent [n_entries].  Deterministic.
 * Eligible are the VECTOR factors without any of the LPMP_ERR_UNSUPPORTED shapes above; the others are left out and counted in
 * *n_left_out.  One group: the eligible unaries that no earlier group holds are visited in ascending index, then the others in
 * ascending index; a union-find runs over the group's members, and a unary joins unless two of its links, parallel factors
 * included, lead into the same component of the group.  Groups are added until every eligible unary is in one, or until max_groups
 * (0: no limit).  Every tree is rooted at a centre (the lower factor index where there are two): its height is
 * ceil(diameter / 2).  At most floor(D / 2) + 1 groups are needed, D the largest number of links of an eligible unary: a unary
 * that is still uncovered and is refused by a group sees at least two of its links become covered in that group. */
int lpmp_plan_suggest_forests(lpmp_plan* p, int64_t max_groups, int64_t* n_groups, int64_t* n_entries, int64_t* group_off, int32_t* unaries,
                              int32_t* parent, int64_t* n_left_out);

int64_t lpmp_dual_size(const lpmp_engine* e);
/* serialize_dual + save_archive / load_archive (include/serialization.hxx:228-424): packed duals */
int lpmp_download_duals(lpmp_engine* e, double* host_out);
/* lpmp_upload_duals settles first, marks all tracked bounds stale and leaves the primal labels as they are (lpmp_evaluate_primal
 * prices them on the duals of the moment), as do lpmp_set_vectors and lpmp_zero_pairwise_duals: only a change of CONSTANTS
 * (lpmp_upload_costs, lpmp_upload_shared_pool, lpmp_set_constants) and lpmp_upload_model unset the labels. */
int lpmp_upload_duals(lpmp_engine* e, const double* host_in);
/* ---- new costs on the plan that is already there ---------------------------------------------------------------------------
 * Everything the engine builds before its first pass — order, weights, level schedules, kernel classes, packets, chain plans, the
 * ticket templates of joined passes, mailboxes — is a function of the STRUCTURE of the model; none of it reads a cost.  These calls
 * give a planned model other numbers and plan nothing: lpmp_engine_plan returns the same pointer, every cached schedule, every
 * lpmp_schedule_create id, every lpmp_boundary / lpmp_halo object, the reparametrization mode and type, the speculation depth, the
 * rows-layout and table-precision modes stay and stay valid, and lpmp_schedules_built does not change.
 *
 * lpmp_upload_costs: same structure, other numbers.  const_data / dual_data are packed exactly as lpmp_model.const_data / dual_data
 * of the uploaded model; NULL = leave that half as it is; *_mem says where the array lives.  LPMP_ERR_STATE before the first
 * lpmp_upload_model and when both pointers are NULL.  The data is copied into wherever the engine keeps that half (its own buffer,
 * or the caller's borrowed one); a LPMP_MEM_DEVICE pointer that IS the buffer the engine already reads is not copied ("I rewrote my
 * buffer in place"), only the derived copies are refreshed.
 *   constants given: every engine-private copy is derived again, by the code of the upload — the {scale, offset} cells of SHARED /
 *     DIFF factors (cell offsets and pool untouched), the float tables under LPMP_TABLES_F32 / _F32_ROUND (same refusals, naming the
 *     lowest factor), the table part of the rows.  An LPMP_ERR_UNSUPPORTED from the narrowing leaves the constants unspecified: from
 *     then on every call that would read them (passes, bounds, primal cost) returns LPMP_ERR_STATE until a later lpmp_upload_costs
 *     with constants succeeds, or lpmp_upload_model.  The dual half of the refused call HAS been applied, and a borrowed constant
 *     buffer holds the refused constants (the tables are narrowed out of it).
 *   duals given (cold start): an open batch of passes that ran ahead is dropped without replay.
 *   duals NOT given (warm start): passes that ran ahead are settled first — the duals are those of the pass the caller is at.  The
 *     one exception to "plans nothing": settling replays the passes the caller had asked for, and the joined launch of THAT pass count
 *     is built (and counted by lpmp_schedules_built) if the engine has not run it before — a function of the structure, cached.
 * In every case all tracked per-factor bounds become stale and the primal labels go back to unset (lpmp_evaluate_primal is +inf
 * until a rounding pass has run on the new costs); the kernel-timing accumulators are left alone.
 * The shared pool (lpmp_model.sh_data) is not part of the packed constants and is not touched here: lpmp_upload_shared_pool below
 * replaces its values.  Its entries, their dims, the entry a factor references, like dims, messages, relations or partitions,
 * remain a job for lpmp_upload_model. */
int lpmp_upload_costs(lpmp_engine* e, const double* const_data, int const_mem, const double* dual_data, int dual_mem);
/* theta of the listed VECTOR factors := row i of src (accumulate = 0) or += row i of src (accumulate != 0; one IEEE add per entry).
 * Row i starts at src + i * src_stride and has f_dim0[factors[i]] entries; src_stride may exceed the longest listed vector (one
 * [n, Lmax] cost volume).  factors is a host array; src is host or device (src_mem).  Settles first; addresses the packed dual array
 * (vector factors live only there, also under the rows layout); marks the bounds of the listed factors stale.  LPMP_ERR_INVALID,
 * naming the offender, with the duals untouched: an index out of range, a non-VECTOR factor, a factor listed twice, src_stride
 * smaller than the longest listed vector. */
int lpmp_set_vectors(lpmp_engine* e, int64_t n, const int32_t* factors, const double* src, int64_t src_stride, int src_mem,
                     int accumulate);
/* New VALUES for the shared pool of the planned model: sh_data is packed as lpmp_model.sh_data of the uploaded model (same
 * n_shared_tables, sh_off, dims), host or device memory (sh_mem); a device source is copied to the host first, where the NaN refusal
 * and the band detection read it.  LPMP_ERR_STATE before the first lpmp_upload_model; LPMP_ERR_INVALID for a NULL pointer, a model
 * without a pool, or a NaN entry (naming the table; +inf is allowed, as at the upload) — with nothing changed.  Only two things in
 * a plan read a pool value: that refusal, and the band of every entry a DIFF factor references.  So the call settles passes that
 * ran ahead, runs lpmp_plan_set_shared_pool on the engine's plan, rewrites the pool block of its device copy (band words and values;
 * the {scale, offset} cells do not move) and drops the captured graphs of every schedule with a launch of class diff — a graph holds
 * the kernel choice; it is captured again on the schedule's next run.  The duals are not touched (any duals are a valid
 * reparametrisation of the new costs); all tracked bounds become stale and the primal labels unset, as after lpmp_upload_costs.
 * Plans nothing: the plan handle, lpmp_schedules_built, every lpmp_schedule_create id and boundary / halo object stay.  Returns after
 * its copies have completed. */
int lpmp_upload_shared_pool(lpmp_engine* e, const double* sh_data, int sh_mem);
/* constants of the listed PAIRWISE factors := row i of src.  Row i starts at src + i * src_stride and has
 * as many entries as the factor has constants (lpmp_model.h: DENSE dim0 * dim1, row-major; POTTS, SHARED, DIFF: 1); factors is a host array,
 * src host or device memory (src_mem).  Settles first.  The row goes to every place the sweep kernels read that factor's constants
 * from: the Potts scalar; the first word of a SHARED / DIFF cell AND the scalar of the constants the cell is gathered from (a later
 * lpmp_upload_costs without new constants keeps it); a dense table in the constant buffer — the engine's own or the caller's borrowed
 * one — and, under the rows layout, the table part of the factor's row (not its messages); under LPMP_TABLES_F32 / _F32_ROUND the
 * narrowed floats in the float table and nothing as doubles (a borrowed buffer is not written for tables).  The bounds of the listed
 * factors become stale and the primal labels unset.  n == 0 is a no-op after the checks.
 * LPMP_ERR_INVALID, naming the offender, with nothing written: an index out of range, a VECTOR factor, a factor listed twice,
 * src_stride smaller than the longest listed row.  LPMP_ERR_UNSUPPORTED, naming the lowest factor, when a float mode refuses an entry
 * of a listed table (the refusals of the upload) — checked by a read-only launch over the listed rows BEFORE anything is written:
 * the old costs are whole and passes continue on them (stronger than lpmp_upload_costs, which cannot afford that pass over every
 * table).  Scales are not validated, as at the upload. */
int lpmp_set_constants(lpmp_engine* e, int64_t n, const int32_t* factors, const double* src, int64_t src_stride, int src_mem);
/* both message vectors of every pairwise factor (DENSE, POTTS, SHARED, DIFF) := +0.0.  Settles first; writes the rows under the rows
 * layout and the packed array otherwise; marks all bounds stale.  Asynchronous on the engine's stream like a pass (it reads nothing
 * of the caller's); lpmp_upload_costs and lpmp_set_vectors return after their copies have completed.  A cold start from device data is lpmp_set_vectors(all unaries,
 * replace) + this call; a warm start after a change of unaries is lpmp_set_vectors(changed ones, differences, accumulate). */
int lpmp_zero_pairwise_duals(lpmp_engine* e);
/* ---- moving label windows: duals and shifts carried along on the device ------------------------------------------------
 * A DIFF_SHIFT model gives variable u a WINDOW of labels c_u ... c_u + d_u - 1; the shift of an edge is c_u - c_v + zero.  When the
 * windows move (coarse to fine, frame to frame) theta_u[x] and the message vectors m_s[x] of the adjacent pairwise factors are indexed
 * by the window-relative label x, which now names another absolute label: kept where they are (lpmp_set_constants + a warm start) they
 * are a valid reparametrisation that belongs to the wrong labels.  This call moves them along their label axis and updates the shifts.
 *
 * A window set is a prepared list of n distinct VECTOR factors u_0 ... u_{n-1} of the uploaded model, like an lpmp_readout: its record
 * and link tables are uploaded at create (counted ONCE by lpmp_schedules_built), a move plans and builds nothing.  factors == NULL:
 * every VECTOR factor in ascending index.  It carries the model it was made for and its device; lpmp_destroy does not free it; after
 * the next lpmp_upload_model every move on it is LPMP_ERR_STATE and destroying it stays legal.
 * Supported per listed factor, checked at create: every message of u is LPMP_M_UNARY_PAIRWISE with u as its left factor and a
 * DIFF_SHIFT factor on the right.  LPMP_ERR_UNSUPPORTED naming the lowest offending listed factor: a peer of any other kind (DENSE,
 * POTTS, SHARED, plain DIFF) or a message of another kind; two messages of one unary into one vector; a DIFF_SHIFT factor with two
 * different unaries on one side; more than 512 labels.  LPMP_ERR_INVALID naming the entry: an index out of range, a non-VECTOR factor,
 * a factor listed twice.  Unlisted parts of the model may be anything.
 *
 * lpmp_move_windows: delta[i] (int32, host or device: delta_mem) is the move of listed factor i, |delta[i]| <= 2^20.  delta(f) = delta[i]
 * for a listed factor, 0 for every other; g_u(x) = min(max(x + delta(u), 0), d_u - 1): new label x is old label x + delta, labels that
 * enter the window copy the nearest old end value.
 *   unaries   theta_u'[x] = theta_u[g_u(x)] for every listed u
 *   messages  m_{p,s}'[x] = m_{p,s}[g_u(x)] for every message of a listed u (pairwise factor p, side s); the vector of the other side
 *             is touched only if that unary is listed, too
 *   shifts    every DIFF_SHIFT factor p next to a listed unary, l / r the unary on side 0 / 1 (a side without a unary: delta 0):
 *             delta(l) != delta(r): shift' = (double) clamp(int(shift) + delta(l) - delta(r), -2^30, 2^30), the conversion of
 *             lpmp_model.h; the scale stays.  The value goes to every place lpmp_set_constants writes the shift of a DIFF_SHIFT row to.
 *             delta(l) == delta(r): the factor's constants are not written
 *   costs     cost_old and cost_new (both or neither; one alone is LPMP_ERR_INVALID): the ORIGINAL unary costs of the listed factors
 *             in the old and in the new window, [n, cost_stride] doubles, host or device (cost_mem), cost_stride >= the longest listed
 *             vector.  Then theta_u'[x] = theta_u[g] + (cost_new_i[x] - cost_old_i[g]), g = g_u(x): the inner difference first; where
 *             the two entries compare equal (==, two +inf included) the term is skipped and theta is carried bit for bit.  Any other
 *             non-finite entry is outside the contract (lpmp_set_vectors afterwards).
 * theta_u[x] + sum_p m_{p,s}[x] is the original unary and every term moves by the same g_u; cost(a, b) = scale * D[clip(a - b + s)] is
 * the same function of the ABSOLUTE labels exactly when s' = s + delta(l) - delta(r): every labelling whose absolute labels lie in
 * both the old and the new windows keeps its reparametrised energy term by term, bit for bit.  All delta 0 and no costs: no byte of
 * duals or constants changes.
 * Settles passes that ran ahead first.  Plans nothing: lpmp_schedules_built does not move, every lpmp_schedule_create id, read-out,
 * boundary / halo object, the mode and the send rule stay valid.  The tracked bounds of the listed unaries and of every adjacent
 * pairwise factor become stale; the primal labels become unset, as after lpmp_set_constants.  With device inputs the call is
 * asynchronous on the engine's stream like a pass; with a host input it returns after its copies.  A host delta out of range is
 * LPMP_ERR_INVALID, naming the entry, with nothing written; a device delta is saturated to +-2^20 where it is read.  LPMP_ERR_STATE
 * before an upload, on a set made for a model that has been replaced since, and while the constants are unspecified. */
typedef struct lpmp_window_set lpmp_window_set;
int lpmp_window_set_create(lpmp_engine* e, int64_t n, const int32_t* factors, lpmp_window_set** out);
void lpmp_window_set_destroy(lpmp_window_set* ws);
int64_t lpmp_window_set_n(const lpmp_window_set* ws);            /* listed factors */
int32_t lpmp_window_set_max_labels(const lpmp_window_set* ws);   /* longest listed vector */
int64_t lpmp_window_set_n_pairwise(const lpmp_window_set* ws);   /* DIFF_SHIFT factors whose shift a move may write */
int lpmp_move_windows(lpmp_engine* e, lpmp_window_set* ws, const int32_t* delta, int delta_mem, const double* cost_old,
                      const double* cost_new, int64_t cost_stride, int cost_mem);
/* lpmp_move_windows that CARRIES the labels instead of unsetting them.  Same arguments, same checks; everything lpmp_move_windows does
 * to duals, shifts, tracked bounds and the caller's arrays, bit for bit.  The labelling is the one piece of state whose meaning is
 * exactly an absolute label:
 *   a listed unary i with a label x < d gets x' = min(max(x - delta_i, 0), d - 1), delta_i saturated as in the move; x == d (unset)
 *   stays unset; unlisted unaries keep their labels.  Afterwards the pairwise slots follow their unaries as after a decode (on a
 *   model the rounding code refuses: unaries only).  When no primal array exists, none is created.
 * Consequence: a labelling whose absolute labels all lie in the old and the new windows keeps its primal cost (lpmp_evaluate_primal)
 * bit for bit, for a move without costs or with cost_old / cost_new that agree on the shared absolute labels — the reparametrised
 * energy is kept term by term, as said above.  A label that left the window names the nearest absolute label that stayed.  The time
 * stamp of the rounding passes stays, as after lpmp_upload_primal.  lpmp_move_windows itself keeps unsetting the labels. */
int lpmp_move_windows_carry(lpmp_engine* e, lpmp_window_set* ws, const int32_t* delta, int delta_mem, const double* cost_old,
                            const double* cost_new, int64_t cost_stride, int cost_mem);
/* host only: the same support check on a plan.  n_links: unary-pairwise links of the listed factors, n_pairwise as above (either may be
 * NULL); why (why_n bytes; may be NULL): "" or the refusal, which lpmp_last_error reports as well */
int lpmp_plan_window_info(lpmp_plan* p, int64_t n, const int32_t* factors, int64_t* n_links, int64_t* n_pairwise, char* why, int why_n);
/* schedules, chain plans and joined-pass templates planned and uploaded for the current model since lpmp_upload_model */
int64_t lpmp_schedules_built(const lpmp_engine* e);

void* lpmp_device_duals(lpmp_engine* e);   /* device pointer of the packed duals (for zero-copy exchange); with the rows layout
                                              the dense pairwise factors' vectors are written out to it first, and the rows are
                                              refreshed from it before the next pass (the caller is assumed to write it) */
/* Rows layout (engine-private): from the NEXT lpmp_upload_model on, every dense pairwise factor lives on the device
 * as one contiguous row [table | m1 | m2] of a buffer of the engine's own, so that the three reads of a receive are one burst
 * (random graphs: C4).  The packed dual array — serialize_dual order, reference factors_messages.hxx:3196-3223 — stays the format
 * of every call that hands duals over (lpmp_download_duals / lpmp_upload_duals / lpmp_device_duals / lpmp_synchronize with a
 * borrowed buffer / the lpmp_boundary_* offsets): the message vectors are copied between the two at those calls, never inside a
 * pass.  Costs the tables a second time in device memory; passes that run ahead of the caller (lpmp_set_speculation) stay off. */
int lpmp_set_rows_layout(lpmp_engine* e, int on);
int lpmp_rows_layout(const lpmp_engine* e);   /* 1 if the uploaded model uses it */

/* Table precision (engine-private): from the NEXT lpmp_upload_model on, every entry of a DENSE pairwise table
 * (LPMP_F_PAIRWISE_DENSE) is stored as a float on the device and widened to double where a kernel loads it.  All arithmetic stays
 * double and in the same order, so the result is bit for bit what the engine computes on the model whose tables are the widened
 * floats — exact for the cost volumes and learned potentials that are float32 where they are produced.  Halves the bytes of the
 * tables in device memory and per pass.  Potts scalars, SHARED / DIFF scales, the shared pool and all duals stay doubles.
 *   LPMP_TABLES_F64        doubles, the default
 *   LPMP_TABLES_F32        strict: the upload returns LPMP_ERR_UNSUPPORTED when an entry x has (double)(float)x != x
 *   LPMP_TABLES_F32_ROUND  entries are rounded to nearest even
 * Both f32 modes refuse (LPMP_ERR_UNSUPPORTED) a finite entry that overflows float and a nonzero one of magnitude below FLT_MIN;
 * the message names the lowest factor index that holds such an entry.  +-inf pass through (hard constraints); NaN is outside the
 * contract as it is for doubles.  From host memory (LPMP_MEM_HOST) the tables pass through a staging buffer of at most 256 MiB
 * and are never resident as doubles; from a caller's device buffer they are narrowed out of it, and afterwards the engine reads
 * only the other factors' constants from that buffer.  Cannot be combined with the rows layout (LPMP_ERR_UNSUPPORTED at the
 * upload).  The lpmp_boundary_* / lpmp_halo_* kernels touch duals only and work unchanged. */
enum lpmp_table_precision_mode { LPMP_TABLES_F64 = 0, LPMP_TABLES_F32 = 1, LPMP_TABLES_F32_ROUND = 2 };
int lpmp_set_table_precision(lpmp_engine* e, int precision);
int lpmp_table_precision(const lpmp_engine* e);   /* what the uploaded model uses */
/* the same for a stand-alone plan: only the byte accounting of the schedules planned from now on changes (4 instead of 8 bytes per
 * dense table entry: algorithmic bytes, band and tile sizes of the Infinity-Cache order, the heavy-launch rule); kernel classes,
 * levels and records are those of the f64 plan */
int lpmp_plan_set_table_precision(lpmp_plan* p, int precision);

/* Persistent launches (the chain executor and the joined passes in Infinity-Cache order) assume that resident
 * workgroups keep running, i.e. that the device is this process's own.  When several processes time-share one device its scheduler
 * switches queues, ticket holders freeze while their waiters poll, and a run may end in LPMP_ERR_DEVICE ("a dependency wait timed
 * out") with the duals undefined.  A host that shares its device (lpmp_device_identity tells) switches them off for its engine:
 * every schedule then runs launch by launch / as a replayed graph — same results, bit for bit.  Default on; LPMP_NO_CHAIN=1 /
 * LPMP_NO_BLOCKED_PASSES=1 in the environment keep them off whatever is set here.  Callable at any time. */
int lpmp_set_persistent_launches(lpmp_engine* e, int on);
int lpmp_persistent_launches(const lpmp_engine* e);   /* 1 if on */
/* "pci=<domain:bus:device.function> uuid=<hex>" of HIP device ordinal `device` (NUL-terminated, cap >= 64): equal strings = one
 * physical GPU, also when every process has a visibility mask of its own and all of them call their device "0" */
int lpmp_device_identity(int device, char* out, int64_t cap);

const lpmp_plan* lpmp_engine_plan(const lpmp_engine* e);
lpmp_plan* lpmp_engine_plan_mut(lpmp_engine* e);

/* kernel timing with HIP events on the engine's stream (bench.py roofline leg).  While enabled every
 * sweep launch is bracketed by an event pair.  Classes: enum KClass in lp_mp_amd/csrc/plan.hpp. */
int lpmp_enable_kernel_timing(lpmp_engine* e, int on);
int lpmp_get_kernel_timing(lpmp_engine* e, int n_classes, double* ms /*[n]*/, int64_t* launches /*[n]*/,
                           int64_t* factors /*[n]*/, int64_t* receives /*[n]*/, int64_t* bytes /*[n]*/);
int lpmp_reset_kernel_timing(lpmp_engine* e);
/* of the launches reported per class: how many were persistent launches of the chain executor */
int lpmp_get_chain_launches(lpmp_engine* e, int n_classes, int64_t* chain_launches /*[n]*/);
/* of the launches reported for class diff: how many ran the banded kernel (sweep_diff_band_kernel) */
int lpmp_get_diff_band_launches(lpmp_engine* e, int64_t* band_launches);
/* ... and how many had a LPMP_F_PAIRWISE_DIFF_SHIFT factor (sweep_diff_shift_kernel or sweep_diff_shift_band_kernel; never
 * sweep_diff_band_kernel) */
int lpmp_get_diff_shift_launches(lpmp_engine* e, int64_t* shift_launches);
/* ... and of those, how many ran the shifted banded kernel (sweep_diff_shift_band_kernel) */
int lpmp_get_diff_shift_band_launches(lpmp_engine* e, int64_t* shift_band_launches);
/* joined-pass launches in the peer-minima form since the last lpmp_reset_kernel_timing; counted with timing off,
 * too (passes that run ahead of the caller are never timed): with timing on since the reset, a part of dense32's chain launches */
int lpmp_get_peer_minima_launches(lpmp_engine* e, int64_t* launches);

/* ---- boundary step of the partitioned (multi-GPU) sweep, DESIGN.md 7 -------------------------------------------------
 * One process per GPU owns one part of the factor graph (lp_mp_amd/multi_gpu.py builds the parts; a C++ host can do
 * the same from lpmp_model arrays).  Cut messages travel as flat runs of doubles between DEVICE buffers the caller
 * owns: the caller posts the exchange itself (RCCL ncclSend / ncclRecv or all-to-all-v on lpmp_engine_stream, or
 * torch.distributed) between these calls.  Every step is the reference's UpdateFactor of a non-owner endpoint restricted
 * to its cut messages (include/factors_messages.hxx:2256-2261), so the whole schedule replays on the unpartitioned
 * model with LP::ComputePass(factorIt, ...) (include/LP_MP.h:981-1005).
 *   out_*   the cut messages this part OWNS (ghost vectors), in exchange order (by peer, then key)
 *   in_*    the cut messages owned elsewhere that end in a variable of this part, in exchange order; in_omega their send
 *           weights (a row sums to <= 1, LP_MP.h:1008-1014); in_order = indices into in_* grouped by variable and, inside
 *           a variable, in the order its message list holds them (receives and sends happen in that order) */
typedef struct lpmp_boundary lpmp_boundary;
int lpmp_boundary_create(lpmp_engine* e, int64_t n_out, const int64_t* out_dual_off, const int32_t* out_len, int64_t n_in,
                         const int64_t* in_dual_off, const int32_t* in_len, const double* in_omega, const int64_t* in_order,
                         lpmp_boundary** out);
void lpmp_boundary_destroy(lpmp_boundary* b);
int64_t lpmp_boundary_out_doubles(const lpmp_boundary* b);   /* size of the send buffer of pack / the buffer of fold */
int64_t lpmp_boundary_in_doubles(const lpmp_boundary* b);    /* size of the receive buffer / the reply buffer */
/* owner: send[...] = ghost vectors (after the ghost receive schedule ran), ghosts zeroed */
int lpmp_boundary_pack(lpmp_engine* e, lpmp_boundary* b, double* send_dev);
/* non-owner: theta += received (list order); reply = omega * theta after all receives; theta -= reply (list order) */
int lpmp_boundary_reply(lpmp_engine* e, lpmp_boundary* b, const double* recv_dev, double* reply_dev);
/* owner: ghost vectors = reply (then run the ghost send schedule) */
int lpmp_boundary_fold(lpmp_engine* e, lpmp_boundary* b, const double* back_dev);
void* lpmp_engine_stream(lpmp_engine* e);                    /* the hipStream_t all engine work is issued on */

/* ---- halos of the lock-step partitioned sweep, DESIGN.md 7 (lp_mp_amd/lockstep.py) ------------------------------------
 * Several ranks execute THE unpartitioned sweep (LP::ComputePass, include/LP_MP.h:981-1005) level by level; between two runs of
 * levels (lpmp_schedule_run) a rank ships the message vectors it wrote that the next run reads on other ranks.  No arithmetic:
 * pack copies the listed vectors of the dual array into a contiguous DEVICE buffer in exchange order, unpack copies a received
 * buffer into the listed vectors; the caller posts the exchange in between (ncclSend / ncclRecv, all-to-all-v) on
 * lpmp_engine_stream.  Vectors are (offset into the packed dual array = serialize_dual order, length) pairs. */
typedef struct lpmp_halo lpmp_halo;
int lpmp_halo_create(lpmp_engine* e, int64_t n_out, const int64_t* out_dual_off, const int32_t* out_len, int64_t n_in,
                     const int64_t* in_dual_off, const int32_t* in_len, lpmp_halo** out);
void lpmp_halo_destroy(lpmp_halo* h);
int64_t lpmp_halo_out_doubles(const lpmp_halo* h);           /* size of the buffer pack fills */
int64_t lpmp_halo_in_doubles(const lpmp_halo* h);            /* size of the buffer unpack reads */
int lpmp_halo_pack(lpmp_engine* e, lpmp_halo* h, double* send_dev);
int lpmp_halo_unpack(lpmp_engine* e, lpmp_halo* h, const double* recv_dev);

/* synthetic workloads: out[i] = u01(splitmix64(seed + (first+i+1)*GOLDEN)) written on the device */
int lpmp_synth_fill(void* device_ptr, int64_t n, uint64_t seed, uint64_t first, void* hip_stream);
/* the same for n_blocks blocks of block_len values each, block b continuing the stream at first_dev[b] (device array):
 * a rank's scattered share of a global cost stream */
int lpmp_synth_fill_blocks(void* device_ptr, int64_t n_blocks, int64_t block_len, uint64_t seed, const int64_t* first_dev, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* LPMP_ENGINE_H */
