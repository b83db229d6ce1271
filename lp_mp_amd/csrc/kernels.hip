// kernels.hip — hand-written gfx950 (CDNA4) kernels of the LP_MP dual block-coordinate-ascent sweep.
//
// What one launch does: every wavefront (or sub-wave lane group) takes ONE updated factor of the
// current level and executes the reference's FactorContainer::UpdateFactor on it
// (reference include/factors_messages.hxx:2256-2261): pull a weight-1 message through every active
// receiving message, then push omega-weighted messages through every active sending message, all
// computed from the factor state after the receives (the reference's tmp_factor copy, :2799-2805).
// Factors of one level touch disjoint memory (plan.cpp, level scheduling), so the result equals the
// sequential sweep of LP::ComputePass (reference include/LP_MP.h:981-1005).
//
// The inner op is min-plus over doubles: no MFMA.  The kernels are HBM-bound streams of pairwise
// tables (dense) or short vectors (Potts); they are built around coalesced 16-B-per-lane loads of the
// tables, LDS staging of the label vectors, and DPP / permute min-reductions inside 64-wide waves.
// All arithmetic is IEEE double without contraction (-ffp-contract=off) so that duals are
// bit-identical to the sequential CPU semantics (min and + are exact; evaluation order is copied).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include <type_traits>

#include "kernels.hpp"

namespace lpmp {

#define LPMP_INF (__builtin_inf())
constexpr int GEN_WAVES = 4;         // (GEN_MAXD, GEN_ADAPTIVE_SENDS: kernels.hpp)

// Tracked lower bounds.  lb[f] holds FactorContainer::LowerBound of factor f, or NaN when it has to be
// recomputed.  A sweep kernel knows the bound of every factor it touches for free:
//   own vector factor            min(theta) after the update
//   pairwise peer after a receive on side s:  min_x (m_s_new[x] + q[x]) with q the min-marginal part it just
//                                computed  ( = min_a (m1[a] + min_b (T[a][b] + m2[b])), reference LP_MP.h:1507-1518 )
//   pairwise peer after a send   unknown without a table scan -> NaN
// so LP::LowerBound after a pass is a sum over an array instead of another read of all tables.
#define LPMP_NAN (__builtin_nan(""))

// Loads / stores of data that is touched once per launch and is far larger than L2 + Infinity Cache (tables and
// message vectors of an HBM-sized model): non-temporal, so that they do not displace anything and the memory
// pipeline does not try to keep them (measured on C3: -5 % time with nt table loads, -8 % with the vectors too).
// NT = false for cache-resident models (C2: the whole state lives in the Infinity Cache between launches).
template <bool NT, class T> __device__ __forceinline__ T ld_stream(const T* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p); else return *p;
}
template <bool NT, class T> __device__ __forceinline__ void st_stream(T* p, T v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p); else *p = v;
}
// Access policy of the DUALS (theta, message vectors).  ACC_PLAIN / ACC_NT: one launch per level, the launch boundary
// makes other workgroups' stores visible.  ACC_COH: the chain executor below — updates of different levels run inside
// ONE launch and hand their results over through flags, so every dual load / store is an agent-scope access
// (global_load / global_store ... sc1: write-through stores, loads that do not hit a stale line of this CU's L1; the
// XCDs' L2s are not coherent with each other, MI355X_MICROARCH.md "inter-workgroup visibility").  The pairwise tables
// are constants and keep the streaming policy in every mode.
// ACC_WG: the level loop below — one WAVE hands values from level to level: loads that do not stop at this CU's L1 (sc0).
enum Access : int { ACC_PLAIN = 0, ACC_NT = 1, ACC_COH = 2, ACC_WG = 3 };
template <int A> __device__ __forceinline__ double ld_dual(const double* p) {
  if constexpr (A == ACC_COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else if constexpr (A == ACC_WG) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else if constexpr (A == ACC_NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <int A> __device__ __forceinline__ void st_dual(double* p, double v) {
  if constexpr (A == ACC_COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else if constexpr (A == ACC_NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// tracked lower bounds: several updates of ONE launch may write the same slot in the chain executor (a factor is
// touched at several levels); plain stores from different XCDs would reach memory in no particular order
template <int A> __device__ __forceinline__ void st_lb(double* p, double v) {
  if constexpr (A == ACC_COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else *p = v;
}

// ---- chain executor: dependent levels inside one persistent launch -------------------------------------------------
// A deep schedule (row-major grids: one level per anti-diagonal; chains of tiny factors) is latency-bound when every
// level is its own launch.  Here the workgroups of ONE launch take "tickets" — blocks of records, numbered in level
// order — from a global counter.  A ticket names the tickets that hold its records' predecessors (the last earlier
// update of every factor it touches, from the host's level analysis); the workgroup requests everything constant
// (packet, pairwise tables) first, THEN waits for those tickets' completion flags, then loads the duals.  A ticket
// only ever waits for lower tickets, and those are held by workgroups that are already running, so the scheme needs
// no assumption about residency or dispatch order.  Every wait is bounded: on a timeout the launch sets an abort word
// and drains, and the host reports an error instead of hanging the device.
// What it DOES assume: the workgroups that are resident keep running — the device is this process's.  When several
// processes oversubscribe one device, its scheduler time-slices their queues XCD by XCD: workgroups of this launch that
// hold tickets can be switched out on one XCD for as long as another process's persistent launch runs there, while the
// workgroups on the other XCDs poll for those tickets — and that other launch may be waiting the same way for an XCD this
// one occupies.  Measured (round 4, 8 rank processes sharing the one GPU of the test box, profiles/r04_8rank_stall_*):
// about every third run stalled until the bound below ended it, every load and barrier of the stalled workgroups frozen
// for exactly as long, neither slower polls nor a read-modify-write publish changed it.  One process per device (what the
// engine is built for) never has this; drivers that put several ranks on one device for smoke runs switch the
// persistent launches off (bench.py; LPMP_NO_CHAIN=1 LPMP_NO_BLOCKED_PASSES=1).
// (ChainArgs, ChainLaunch and HIST_*: kernels.hpp)
// debugging (LPMP_LEVEL_TRACE, engine.cpp): time stamps of the first LEVEL_TRACE_MAX levels of a level-loop launch, 8 slots per level
__device__ long long* g_level_trace = nullptr;
__device__ __forceinline__ void level_stamp(int slot) {
  long long* p = g_level_trace;
  if (p && threadIdx.x == 0) { const long long l = p[0]; if (l < LEVEL_TRACE_MAX) p[8 + 8 * l + slot] = (long long)__builtin_amdgcn_s_memrealtime(); }
}
__device__ __forceinline__ void level_stamp_of(int slot, int tid) {   // the same from another thread (the wave that runs ahead: slots 6, 7)
  long long* p = g_level_trace;
  if (p && (int)threadIdx.x == tid) { const long long l = p[0]; if (l < LEVEL_TRACE_MAX) p[8 + 8 * l + slot] = (long long)__builtin_amdgcn_s_memrealtime(); }
}
__device__ __forceinline__ void chain_stamp(const ChainArgs& ca, int ticket, int k) {
  if (ca.trace && threadIdx.x == 0) ca.trace[8 * (int64_t)ticket + k] = (long long)__builtin_amdgcn_s_memrealtime();
}
// a wait gives up when it has lasted ChainArgs::timeout_ticks (the clock is first read after 1024 polls: short waits never
// read it) or when another wait of the launch has given up
__device__ __forceinline__ bool chain_wait_expired(const ChainArgs& ca, int spins, long long& t0, bool& own) {
  own = false;
  if ((spins & 1023) != 0) return false;
  if (__hip_atomic_load(ca.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return true;
  const long long now = (long long)__builtin_amdgcn_s_memrealtime();
  if (spins == 1024) { t0 = now; return false; }
  own = now - t0 > ca.timeout_ticks;
  return own;
}
// Pause between two polls of a flag or granule.  Constant and short, whatever the age of the wait: in a deep chain the ticket
// that has waited longest is the one next in line, so a pause that grows with the wait lands on the critical path (round 4:
// a back-off to ~4 us after 256 polls made the 512 x 512 8-label Potts grid in row-major order 7.6 instead of 5.8 ms per
// pass, and did nothing for the stalls of a device shared by several processes it was tried against).
__device__ __forceinline__ void chain_poll_pause(int) { __builtin_amdgcn_s_sleep(1); }
// the wait that gives up FIRST says what it was waiting for (abort_flag[1 ...]: engine.cpp puts it into the error message)
__device__ __forceinline__ void chain_abort(const ChainArgs& ca, bool own, int ticket, int dep, int seen, long long t0) {
  if (own && atomicCAS(ca.abort_flag + 1, 0, 1) == 0) {
    const long long now = (long long)__builtin_amdgcn_s_memrealtime();
    ca.abort_flag[2] = ticket; ca.abort_flag[3] = dep; ca.abort_flag[4] = seen; ca.abort_flag[5] = ca.epoch;
    ca.abort_flag[6] = (int)(unsigned)now; ca.abort_flag[7] = (int)(now >> 32); ca.abort_flag[8] = (int)(unsigned)t0; ca.abort_flag[9] = (int)(t0 >> 32);
    ca.abort_flag[10] = __hip_atomic_load(ca.next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __hip_atomic_store(ca.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// template ticket and copy of a ticket of a periodic launch (ChainArgs::per_*)
struct TicketRef { int idx, copy; };
__device__ __forceinline__ TicketRef chain_ticket_ref(const ChainArgs& ca, int ticket) {
  if (ca.per_len == 0 || ticket < ca.per_begin) return {ticket, 0};
  const int q = min((ticket - ca.per_begin) / ca.per_len, ca.per_count - 1);
  return {ticket - q * ca.per_len, q};
}
__device__ __forceinline__ bool chain_flag_set(const ChainArgs& ca, int dep_ticket) {
  if (ca.ring == 0) return __hip_atomic_load(ca.done + dep_ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ca.epoch;
  const int v = __hip_atomic_load(ca.done + dep_ticket % ca.ring, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return (v >> CHAIN_GEN_BITS) == ca.epoch && (v & ((1 << CHAIN_GEN_BITS) - 1)) >= dep_ticket / ca.ring;
}
// all threads of the workgroup; returns false when the run was aborted
__device__ __forceinline__ bool chain_wait(const ChainArgs& ca, int ticket) {
  __shared__ int s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  const TicketRef tr = chain_ticket_ref(ca, ticket);
  const int b = ca.dep_off[tr.idx], e = ca.dep_off[tr.idx + 1];
  const int shift = tr.copy * ca.per_len;
  // ring: the slot this ticket will publish into must hold its previous occupant's completion (ticket - ring)
  const int extra = (ca.ring > 0 && ticket >= ca.ring) ? 1 : 0;
  for (int i = b + (int)threadIdx.x; i < e + extra; i += (int)blockDim.x) {
    const int d = i < e ? ca.dep[i] + shift : ticket - ca.ring;
    int spins = 0; long long t0 = 0; bool own;
    while (!chain_flag_set(ca, d)) {
      chain_poll_pause(spins);
      if (chain_wait_expired(ca, ++spins, t0, own)) {
        chain_abort(ca, own, ticket, d, __hip_atomic_load(ca.done + (ca.ring ? d % ca.ring : d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), t0);
        s_bad = 1;
        break;
      }
    }
  }
  __syncthreads();
  chain_stamp(ca, ticket, 1);                      // predecessors seen
  return s_bad == 0;
}
// all threads: every wave drains its stores, then one lane publishes the ticket.
// MEMORY-MODEL INVARIANT (why relaxed flags suffice, and what must stay true): the hand-over is not a release / acquire
// pair — at agent scope that would write back and invalidate the whole L2 of the XCD per ticket — but rests on three
// properties of the accesses themselves: (1) every dual load / store and every tracked-bound store of a chain body is an
// agent-scope atomic (sc1: stores write through to memory, loads do not hit a possibly stale L2 / L1 line) — enforced by
// the static_asserts `!CHAIN || A == ACC_COH` in the bodies; (2) a wave's stores have left the CU when its vmcnt reaches
// 0 (`s_waitcnt vmcnt(0)` below, then the workgroup barrier, then the flag store); (3) the waiting side reads duals only
// after it has seen the flag (chain_wait returns, then load_own_and_targets).  Data that is NOT accessed this way must
// not cross tickets: rounded labels (store_label) are written and read by the record of the SAME factor only, pairwise
// tables and packets are constants.
__device__ __forceinline__ void chain_publish(const ChainArgs& ca, int ticket) {
  chain_stamp(ca, ticket, 2);                      // body done, stores issued
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    if (ca.ring == 0) __hip_atomic_store(ca.done + ticket, ca.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_store(ca.done + ticket % ca.ring, (ca.epoch << CHAIN_GEN_BITS) | (ticket / ca.ring), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  chain_stamp(ca, ticket, 3);                      // published
}

// ---- tickets ahead (chain_loop_roles_ahead, chain_dense_pq_ahead_kernel) -----------------------------------------------------------
// What chain_wait collects in dependent round trips — dep_off[idx], then dep[i], then the flag — a ticket of that loop has in LDS
// when it begins: its descriptor (ChainAhead::desc, plan.hpp ticket_descriptors), fetched by wave 0 during the ticket before.  The
// wait is therefore split: chain_poll_issue requests the FIRST poll of every predecessor's flag right behind the packet request,
// chain_wait_polled looks at the answers after the tables have been requested and keeps polling only where a flag was not yet set.
// The same bounds and abort words as chain_wait; the invariant above chain_publish holds as it stands: descriptors and packets are
// constants written before the launch (plain loads), flags take agent-scope loads, duals are requested after the flags were seen.
struct PqAhead {
  const ChainAhead* aa;     // the launch's descriptors
  const int* desc;          // LDS: this ticket's descriptor
  int copy;                 // its copy of the period (chain_ticket_ref)
  int next;                 // thread 0: the number drawn for the next ticket — the atomic's result, awaited in chain_wait_polled
  int word;                 // lanes 0-15 of wave 0: their word of the next ticket's descriptor, awaited behind the body
  int* s_next;              // LDS: where the next ticket's number goes
  int* s_bad;               // LDS: set by a wait that gave up (the loop clears it behind the publish)
  int d, v;                 // this thread's first predecessor and the flag word of its first poll (d < 0: none)
};
__device__ __forceinline__ int chain_flag_word(const ChainArgs& ca, int dep_ticket) {
  return __hip_atomic_load(ca.done + (ca.ring ? dep_ticket % ca.ring : dep_ticket), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool chain_flag_word_set(const ChainArgs& ca, int dep_ticket, int v) {   // chain_flag_set on a word already read
  if (ca.ring == 0) return v == ca.epoch;
  return (v >> CHAIN_GEN_BITS) == ca.epoch && (v & ((1 << CHAIN_GEN_BITS) - 1)) >= dep_ticket / ca.ring;
}
// predecessor i of the ticket: inline, from dep[] behind the inline ones, or (i == n) the ring predecessor
__device__ __forceinline__ int chain_desc_dep(const ChainArgs& ca, const PqAhead& ah, int ticket, int i, int n, int n_inline) {
  if (i >= n) return ticket - ca.ring;
  const int d = i < n_inline ? ah.desc[TD_DEPS + i] : ca.dep[ah.desc[TD_REST] + (i - n_inline)];
  return d + ah.copy * ca.per_len;
}
// all threads: thread i requests the flag of predecessor i.  A ticket with more dependencies than the descriptor holds inline takes
// the round trip through dep[] here, behind a branch the whole workgroup agrees on, so that the others wait for nothing
__device__ __forceinline__ void chain_poll_issue(const ChainArgs& ca, int ticket, PqAhead& ah) {
  const int n = __builtin_amdgcn_readfirstlane(ah.desc[TD_NDEPS]);
  const int n_inline = min(n, ah.aa->desc_inline);
  const int total = n + ((ca.ring > 0 && ticket >= ca.ring) ? 1 : 0);
  const int i = (int)threadIdx.x;
  ah.d = -1; ah.v = 0;
  if (i < n_inline) ah.d = ah.desc[TD_DEPS + i] + ah.copy * ca.per_len;
  else if (i >= n && i < total) ah.d = ticket - ca.ring;
  if (n > n_inline) { if (i >= n_inline && i < n) ah.d = ca.dep[ah.desc[TD_REST] + (i - n_inline)] + ah.copy * ca.per_len; }
  if (ah.d >= 0) ah.v = chain_flag_word(ca, ah.d);
}
// all threads; returns false when the run was aborted.  Behind the barrier wave 0 takes the next ticket's number, which the atomic
// has had the whole wait to return, puts it down for the next iteration and requests that ticket's descriptor, a word per lane
__device__ __forceinline__ bool chain_wait_polled(const ChainArgs& ca, int ticket, PqAhead& ah) {
  const int n = __builtin_amdgcn_readfirstlane(ah.desc[TD_NDEPS]);
  const int n_inline = min(n, ah.aa->desc_inline);
  const int total = n + ((ca.ring > 0 && ticket >= ca.ring) ? 1 : 0);
  bool first = true;
  // (a second trip of this loop, through chain_desc_dep, needs a ticket with more predecessors than the workgroup has threads: no
  // template the planner builds has one — the headline's tickets have at most 8 and the ring's — and no test reaches it.  It is
  // kept, with chain_wait's striding, so that the descriptor format sets no cap of its own on a ticket's dependency count)
  for (int i = (int)threadIdx.x; i < total; i += (int)blockDim.x) {
    const int d = first ? ah.d : chain_desc_dep(ca, ah, ticket, i, n, n_inline);
    bool set = first ? chain_flag_word_set(ca, d, ah.v) : chain_flag_set(ca, d);
    first = false;
    int spins = 0; long long t0 = 0; bool own;
    while (!set) {
      chain_poll_pause(spins);
      if (chain_wait_expired(ca, ++spins, t0, own)) {
        chain_abort(ca, own, ticket, d, chain_flag_word(ca, d), t0);
        *ah.s_bad = 1;
        break;
      }
      set = chain_flag_set(ca, d);
    }
  }
  __syncthreads();
  chain_stamp(ca, ticket, 1);                      // predecessors seen
  if (threadIdx.x < 64) {
    const int nt = __builtin_amdgcn_readfirstlane(ah.next);
    if (threadIdx.x == 0) *ah.s_next = nt;
    if (nt < ca.n_tickets && threadIdx.x < TICKET_DESC_WORDS) ah.word = ah.aa->desc[(int64_t)chain_ticket_ref(ca, nt).idx * TICKET_DESC_WORDS + threadIdx.x];
  }
  return *ah.s_bad == 0;
}


// Mailbox of a dense chain (chain_plan.cpp decides which vectors travel this way): the value a send has just computed, as two
// self-validating 8-byte granules {half of the double, epoch of the running launch}.  An aligned 8-byte access is atomic,
// so a granule whose tag is this launch's epoch IS the producer's value — no ordering with any other store is needed, and
// the consumer has the value after ONE trip instead of two (completion flag seen, then the vector fetched).  What the
// consumer may conclude from a granule is only this value: the producer's other stores are not yet visible, which is why
// chain_plan.cpp keeps a flag dependency wherever anything else of the producer is read or overwritten.
__device__ __forceinline__ void mailbox_put(unsigned long long* q, double v, int epoch) {
  const unsigned long long tag = (unsigned long long)(unsigned)epoch << 32;
  __hip_atomic_store(q, tag | (unsigned)__double2loint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(q + 1, tag | (unsigned)__double2hiint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double mailbox_take(const ChainArgs& ca, const unsigned long long* q, bool& bad) {
  const unsigned tag = (unsigned)ca.epoch;
  long long t0 = 0;
  for (int spins = 0;;) {
    const unsigned long long a = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long b = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((unsigned)(a >> 32) == tag && (unsigned)(b >> 32) == tag) return __hiloint2double((int)(unsigned)b, (int)(unsigned)a);
    chain_poll_pause(spins);
    bool own;
    if (chain_wait_expired(ca, ++spins, t0, own)) {
      chain_abort(ca, own, -1, -2, (int)(__hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32), t0);   // a mailbox granule
      bad = true;
      return 0.0;
    }
  }
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double shfl_xor_f64(double v, int mask) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_xor(lo, mask, 64);
  hi = __shfl_xor(hi, mask, 64);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmin(v, shfl_xor_f64(v, m));
  return v;
}


// min all-reduce over aligned groups of CL lanes (CL <= 16) with DPP moves: no LDS-crossbar round trip.
// quad_perm [1,0,3,2] and [2,3,0,1] pair lanes inside a quad, row_half_mirror / row_mirror pair quads and
// half rows; for a min it only matters that every step pairs the two halves that are still missing.
template <int CTRL>
__device__ __forceinline__ double dpp_mov_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
template <int CL>
__device__ __forceinline__ double row_allreduce_min(double v) {
  static_assert(CL == 2 || CL == 4 || CL == 8 || CL == 16, "row width");
  v = fmin(v, dpp_mov_f64<0xB1>(v));                       // lane ^ 1
  if constexpr (CL >= 4) v = fmin(v, dpp_mov_f64<0x4E>(v));   // lane ^ 2
  if constexpr (CL >= 8) v = fmin(v, dpp_mov_f64<0x141>(v));  // row_half_mirror: other quad of the 8
  if constexpr (CL >= 16) v = fmin(v, dpp_mov_f64<0x140>(v)); // row_mirror: other half of the 16
  return v;
}
// fmin as ONE v_min_f64.  In front of an fmin whose operand arrived through a DPP move or a shuffle the compiler puts a
// canonicalising v_max_f64 x, x (it cannot see where the bits come from); that changes a signalling NaN only, and the callers hold
// none: sums and minima of table entries and duals.  (A DPP move that reads the result still gets its wait states: the hazard
// check counts any instruction that defines the register, an asm statement included — seen in the assembly.)
__device__ __forceinline__ double fmin_raw(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// One halving exchange of a min reduce-scatter inside a 16-lane row.  CTRL pairs every lane of the banks (groups of 4 lanes) in
// LO_BANKS with a lane of the other banks.  The LO lanes keep `lo` and take their partner's `lo`, the others keep `hi` and take
// their partner's `hi`: two DPP moves per half under complementary bank masks — a lane whose bank is masked out keeps `old`, its own
// value of the operand it keeps — so both halves end with min(kept, received) without a select.
template <int CTRL, int LO_BANKS>
__device__ __forceinline__ double dpp_halve_min(double lo, double hi) {
  constexpr int HI_BANKS = 0xF & ~LO_BANKS;
  const int l0 = __double2loint(lo), l1 = __double2hiint(lo), h0 = __double2loint(hi), h1 = __double2hiint(hi);
  const int a0 = __builtin_amdgcn_update_dpp(h0, l0, CTRL, 0xF, LO_BANKS, false);   // LO lanes: received, others: kept
  const int a1 = __builtin_amdgcn_update_dpp(h1, l1, CTRL, 0xF, LO_BANKS, false);
  const int b0 = __builtin_amdgcn_update_dpp(l0, h0, CTRL, 0xF, HI_BANKS, false);   // LO lanes: kept, others: received
  const int b1 = __builtin_amdgcn_update_dpp(l1, h1, CTRL, 0xF, HI_BANKS, false);
  return fmin_raw(__hiloint2double(a1, a0), __hiloint2double(b1, b0));
}
template <int G, int L>
__device__ __forceinline__ double vec_min(double v) {   // min over the first L lanes of a G-lane group (others pass +inf)
  constexpr int W = L < G ? L : G;
  v = row_allreduce_min<(W < 16 ? W : 16)>(v);
  if constexpr (W > 16) v = fmin(v, shfl_xor_f64(v, 16));
  if constexpr (W > 32) v = fmin(v, shfl_xor_f64(v, 32));
  return v;
}

// MaximizePotentialAndComputePrimal of a vector factor held one element per lane (first `valid` lanes of a G-lane
// group, padded width W): index of the FIRST minimum, like std::min_element (reference test/test_model.hxx:27-33)
template <int G, int W>
__device__ __forceinline__ int group_argmin(double v, bool valid, int g) {
  const double x = valid ? v : LPMP_INF;
  const double mn = vec_min<G, W>(x);
  const unsigned long long hit = __ballot(valid && x == mn);
  const int base = (int)(threadIdx.x & 63) - g;
  const unsigned long long gm = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << base;
  return __ffsll((long long)(hit & gm)) - 1 - base;
}
// the label is only taken when the factor has none yet (primal_ unset = label count)
__device__ __forceinline__ void store_label(int32_t* __restrict__ primal, int factor, int n_labels, int label) {
  int32_t* pr = primal + 2 * (int64_t)factor;
  if (*pr >= n_labels) *pr = label;
}

// -------------------------------------------------------------------------------------------------
// Generic kernel: any factor kind, any message kind, either role.  Two shapes of the same code:
//   G = 64: one wave per updated factor, state (own duals, snapshot, delta) in LDS, up to GEN_MAXD doubles;
//   G = 1:  one LANE per updated factor for tiny factors (every dim <= SMALL_MAXD: labeling-list edge / triplet
//           factors, two-label toy factors, small pairwise factors that are themselves updated) — 64 factors per
//           wave, no cross-lane step at all, the per-lane state interleaved in LDS ([element][lane]: conflict free).
// -------------------------------------------------------------------------------------------------
constexpr int SMALL_WAVES = 1;
template <int G> struct GenCtx;
template <> struct GenCtx<64> {
  static constexpr int STRIDE = 64, FPB = GEN_WAVES, THREADS = 64 * GEN_WAVES;
  static constexpr int MAX_ADAPTIVE_SENDS = GEN_ADAPTIVE_SENDS;
  struct Lds { double own[GEN_MAXD]; double snap[GEN_MAXD]; double dl[GEN_MAXD]; double imp[GEN_ADAPTIVE_SENDS]; };
  Lds& s; const int lane;
  __device__ __forceinline__ double& imp(int i) const { return s.imp[i]; }
  __device__ __forceinline__ double& own(int i) const { return s.own[i]; }
  __device__ __forceinline__ double& snap(int i) const { return s.snap[i]; }
  __device__ __forceinline__ double& dl(int i) const { return s.dl[i]; }
  __device__ __forceinline__ int first() const { return lane; }
  __device__ __forceinline__ bool leader() const { return lane == 0; }
  __device__ __forceinline__ static double gmin(double v) { return wave_min(v); }
  __device__ __forceinline__ static int gmin(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
  }
  __device__ __forceinline__ static void sync() { wave_sync(); }
};
template <> struct GenCtx<1> {
  static constexpr int STRIDE = 1, FPB = 64 * SMALL_WAVES, THREADS = 64 * SMALL_WAVES;
  static constexpr int MAX_ADAPTIVE_SENDS = SMALL_MAXD;
  struct Lds { double own[SMALL_MAXD][64]; double snap[SMALL_MAXD][64]; double dl[SMALL_MAXD][64]; double imp[SMALL_MAXD][64]; };
  Lds& s; const int lane;
  __device__ __forceinline__ double& imp(int i) const { return s.imp[i][lane]; }
  __device__ __forceinline__ double& own(int i) const { return s.own[i][lane]; }
  __device__ __forceinline__ double& snap(int i) const { return s.snap[i][lane]; }
  __device__ __forceinline__ double& dl(int i) const { return s.dl[i][lane]; }
  __device__ __forceinline__ int first() const { return 0; }
  __device__ __forceinline__ bool leader() const { return true; }
  __device__ __forceinline__ static double gmin(double v) { return v; }
  __device__ __forceinline__ static int gmin(int v) { return v; }
  __device__ __forceinline__ static void sync() {}
};

// Device placement of a SHARED pairwise factor's constants (engine.cpp, lpmp_upload_model): two 8-byte words
// {scale, offset of its table relative to the const base pointer as an int64}; the table is row-major d0 x d1.
__device__ __forceinline__ int64_t shared_table_off(const double* __restrict__ cdata, int64_t coff) {
  return __double_as_longlong(cdata[coff + 1]);
}
// (a DIFF factor has the same two words: its table is the vector D of d0 + d1 - 1 entries, cost(a, b) = scale * D[a - b + d1 - 1])
// A DIFF_SHIFT factor has four words {scale, offset of D, shift, n}: shift is the double of the constants as the caller wrote it
// (it may never have been on the host), n the length of D as an int64, from the plan.  cost(a, b) = scale * D[clamp(a - b + s, 0, n - 1)]
// with s = diff_shift_int(shift): NaN -> 0, saturated to [-2^30, 2^30], truncated toward zero (include/lpmp_model.h).  |a - b| < 2^16,
// so a - b + s cannot overflow, and the clamp keeps every read inside D whatever the bits of shift are.
__device__ __forceinline__ int diff_shift_int(double shift) {
  const double x = shift == shift ? shift : 0.0;
  return (int)fmin(fmax(x, -1073741824.0), 1073741824.0);
}
__device__ __forceinline__ int diff_shift_n(const double* __restrict__ cdata, int64_t coff) { return (int)__double_as_longlong(cdata[coff + 3]); }
__device__ __forceinline__ int diff_shift_index(int k, int s, int n) { return min(max(k + s, 0), n - 1); }
// pairwise cost T(a,b) of a pairwise factor (dense table, Potts scalar, or scale * shared table / difference vector: ONE multiply,
// so that the factor is bit for bit a dense factor whose table is scale * V)
// t32 (wave-uniform, SWEEP_TAB32): DENSE tables are stored as floats (engine.cpp, table precision) and widened here — every
// other constant stays a double
__device__ __forceinline__ double pw_cost(const double* __restrict__ cdata, int64_t coff, int kind, int d1, int a, int b, int t32) {
  if (kind == LPMP_F_PAIRWISE_DENSE)
    return t32 ? (double)reinterpret_cast<const float*>(cdata + coff)[(int64_t)a * d1 + b] : cdata[coff + (int64_t)a * d1 + b];
  if (kind == LPMP_F_PAIRWISE_SHARED) return cdata[coff] * cdata[shared_table_off(cdata, coff) + (int64_t)a * d1 + b];
  if (kind == LPMP_F_PAIRWISE_DIFF) return cdata[coff] * cdata[shared_table_off(cdata, coff) + (a - b + d1 - 1)];
  if (kind == LPMP_F_PAIRWISE_DIFF_SHIFT)
    return cdata[coff] * cdata[shared_table_off(cdata, coff) + diff_shift_index(a - b, diff_shift_int(cdata[coff + 2]), diff_shift_n(cdata, coff))];
  return a == b ? 0.0 : cdata[coff];
}

// dl[x] = omega * (m_s[x] + min_y (T + m_o[y])) for side s of a pairwise factor whose message vectors are
// read through m (global: live peer, or LDS: own snapshot / live own state)
template <class C, class Src>
__device__ __forceinline__ void pw_min_marginal(const C& c, const double* __restrict__ cdata, int64_t coff, int kind, int d0, int d1,
                                                Src m, int side, double omega, int t32) {
  if (side == 0) {
    for (int a = 0; a < d0; ++a) {
      double v = LPMP_INF;
      for (int b = c.first(); b < d1; b += C::STRIDE) v = fmin(v, pw_cost(cdata, coff, kind, d1, a, b, t32) + m(d0 + b));
      v = C::gmin(v);
      if (c.leader()) c.dl(a) = omega * (m(a) + v);
    }
  } else {
    for (int b = c.first(); b < d1; b += C::STRIDE) {
      double v = LPMP_INF;
      for (int a = 0; a < d0; ++a) v = fmin(v, pw_cost(cdata, coff, kind, d1, a, b, t32) + m(a));
      c.dl(b) = omega * (m(d0 + b) + v);
    }
  }
  C::sync();
}

// labeling_message::compute_msg (reference labeling_list_factor.hxx:411-443): dl[l] = omega*(min_{r:tab[r]==l} R[r] - not_taken)
template <class C, class Src>
__device__ __forceinline__ void labeling_to_left(const C& c, Src R, int nr, const int32_t* __restrict__ tab, int nl, int implicit_origin,
                                                 double omega) {
  double nt = implicit_origin ? 0.0 : LPMP_INF;
  for (int r = 0; r < nr; ++r) if (tab[r] >= nl) nt = fmin(nt, R(r));
  for (int l = c.first(); l < nl; l += C::STRIDE) {
    double v = LPMP_INF;
    for (int r = 0; r < nr; ++r) if (tab[r] == l) v = fmin(v, R(r));
    c.dl(l) = omega * (v - nt);
  }
  C::sync();
}

template <class C, class Src>
__device__ __forceinline__ void minnorm_delta(const C& c, Src src, int n, double omega) {
  double mn = LPMP_INF;
  for (int i = c.first(); i < n; i += C::STRIDE) mn = fmin(mn, src(i));
  mn = C::gmin(mn);
  for (int i = c.first(); i < n; i += C::STRIDE) c.dl(i) = omega * (src(i) - mn);
  C::sync();
}

// FactorContainer::LowerBound of a factor seen through an accessor (its duals as they would be after a send):
// vector factor min_i d(i), clamped at 0 with an implicit origin; pairwise min_a ( m(a) + min_b (T[a][b] + m(d0 + b)) )
template <class C, class Acc>
__device__ __forceinline__ double vec_lb_through(const C& c, int n, Acc d, int implicit_origin) {
  double v = LPMP_INF;
  for (int i = c.first(); i < n; i += C::STRIDE) v = fmin(v, d(i));
  v = C::gmin(v);
  if (implicit_origin && 0.0 < v) v = 0.0;
  return v;
}
template <class C, class Acc>
__device__ __forceinline__ double pw_lb_through(const C& c, const double* __restrict__ cdata, int64_t coff, int kind, int d0, int d1, Acc m, int t32) {
  double best = LPMP_INF;
  for (int a = 0; a < d0; ++a) {
    double v = LPMP_INF;
    for (int b = c.first(); b < d1; b += C::STRIDE) v = fmin(v, pw_cost(cdata, coff, kind, d1, a, b, t32) + m(d0 + b));
    v = C::gmin(v);
    best = fmin(best, m(a) + v);
  }
  return best;
}

// A: access policy of the duals (ACC_COH inside the chain executor)
template <int G, int A>
__device__ __forceinline__ void generic_body(const UpdRec* __restrict__ recs, const Op* __restrict__ ops, double* __restrict__ dual,
                                             const double* __restrict__ cdata, const int32_t* __restrict__ tabs, double* __restrict__ lb,
                                             int32_t* __restrict__ primal, const int32_t* __restrict__ pw_unary, int64_t first, int64_t count,
                                             int flags, int64_t block) {
  using C = GenCtx<G>;
  __shared__ typename C::Lds lds[G == 64 ? GEN_WAVES : SMALL_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t idx = block * C::FPB + (G == 64 ? wave : (int)threadIdx.x);
  if (idx >= count) return;
  const C c{lds[wave], lane};
  const UpdRec rec = recs[first + idx];
  const int t32 = flags & SWEEP_TAB32;
  const int okind = rec.kind_flags & 15;
  const int on = okind == LPMP_F_VECTOR ? rec.d0 : rec.d0 + rec.d1;   // own dual size
  double* own_g = dual + rec.dual_off;
  for (int i = c.first(); i < on; i += C::STRIDE) c.own(i) = ld_dual<A>(own_g + i);
  C::sync();
  if constexpr (G == 1 && A == ACC_WG) { asm volatile("" :: "v"(c.own(0))); level_stamp(1); }

  const int n_ops = rec.n_recv + rec.n_send;
  // delta of one message into c.dl: computed from the peer (receive) or from the snapshot / live own state (send)
  auto compute_delta = [&](const Op& op, const bool recv, const bool live_src, const double omega) {
    const int code = op.info & 15, role = (op.info >> 4) & 1, side = (op.info >> 5) & 1, imp = (op.info >> 6) & 1;
    const int pkind = (op.info >> 8) & 15;
    const double* peer = dual + op.peer_dual;
    const int len = op.len;
    auto from_peer = [&](int i) { return ld_dual<A>(peer + i); };
    auto from_own = [&](int i) { return live_src ? c.own(i) : c.snap(i); };
    const bool by_right = recv ? (role == 0) : (role == 1);
    if (code == OP_UP) {
      if (by_right) {   // min-marginal of the pairwise (right) factor
        if (recv) pw_min_marginal(c, cdata, op.peer_const, pkind, op.pd0, op.pd1, from_peer, side, omega, t32);
        else pw_min_marginal(c, cdata, rec.const_off, okind, rec.d0, rec.d1, from_own, side, omega, t32);
      } else {          // omega * theta of the unary (left) factor
        for (int i = c.first(); i < len; i += C::STRIDE) c.dl(i) = omega * (recv ? ld_dual<A>(peer + i) : from_own(i));
        C::sync();
      }
    } else if (code == OP_LABELING) {
      const int32_t* tab = tabs + op.peer_const;
      if (by_right) {
        if (recv) labeling_to_left(c, from_peer, op.pd0, tab, op.pd1, imp, omega);
        else labeling_to_left(c, from_own, rec.d0, tab, op.pd1, imp, omega);
      } else {
        for (int i = c.first(); i < len; i += C::STRIDE) c.dl(i) = omega * (recv ? ld_dual<A>(peer + i) : from_own(i));
        C::sync();
      }
    } else {            // OP_MINNORM
      if (recv) minnorm_delta(c, from_peer, len, omega);
      else minnorm_delta(c, from_own, len, omega);
    }
  };
  // one receive or send: compute delta, then +delta to the side that did not compute it and -delta to the side that did
  auto run_op = [&](const Op& op, const bool recv, const bool live_src, const double omega) {
    if (c.leader()) st_lb<A>(lb + op.peer, LPMP_NAN);
    const int code = op.info & 15, role = (op.info >> 4) & 1, side = (op.info >> 5) & 1, imp = (op.info >> 6) & 1;
    double* peer = dual + op.peer_dual;
    const int len = op.len;
    [[maybe_unused]] auto from_own = [&](int i) { return live_src ? c.own(i) : c.snap(i); };
    // the message is computed by the peer for a receive and by the updated factor for a send
    const bool by_right = recv ? (role == 0) : (role == 1);
    if constexpr (G == 1) {
      // labeling message with the updated factor on the left (multicut edge variable <-> triplet / quadruple factor),
      // lane-per-factor form: deep schedules of such factors are bound by the chain of dependent loads of ONE
      // update, so the match table and the peer's costs are requested together, unconditionally, as soon as the op
      // is known (2 round trips per op instead of 4) and the reparametrisation reuses the loaded costs.  Same
      // arithmetic as the general path below.
      if (code == OP_LABELING && role == 0) {
        const int32_t* tab = tabs + op.peer_const;
        const int nr = op.pd0, nl = op.pd1;
        int tv[SMALL_MAXD]; double Rv[SMALL_MAXD];
#pragma unroll
        for (int r = 0; r < SMALL_MAXD; ++r) { const bool in = r < nr; tv[r] = in ? tab[r] : nl; Rv[r] = in ? ld_dual<A>(peer + r) : LPMP_INF; }
        if (recv) {
          double nt = imp ? 0.0 : LPMP_INF;
#pragma unroll
          for (int r = 0; r < SMALL_MAXD; ++r) if (tv[r] >= nl) nt = fmin(nt, Rv[r]);   // entries beyond nr hold +inf
          for (int l = 0; l < nl; ++l) {
            double v = LPMP_INF;
#pragma unroll
            for (int r = 0; r < SMALL_MAXD; ++r) if (tv[r] == l) v = fmin(v, Rv[r]);
            c.dl(l) = omega * (v - nt);
          }
          for (int i = 0; i < len; ++i) c.own(i) += +1.0 * c.dl(i);
#pragma unroll
          for (int r = 0; r < SMALL_MAXD; ++r) if (r < nr && tv[r] < nl) st_dual<A>(peer + r, Rv[r] + -1.0 * c.dl(tv[r]));
        } else {
          for (int i = 0; i < len; ++i) c.dl(i) = omega * from_own(i);
          for (int i = 0; i < len; ++i) c.own(i) += -1.0 * c.dl(i);
#pragma unroll
          for (int r = 0; r < SMALL_MAXD; ++r) if (r < nr && tv[r] < nl) st_dual<A>(peer + r, Rv[r] + +1.0 * c.dl(tv[r]));
        }
        return;
      }
    }
    compute_delta(op, recv, live_src, omega);
    // (reference MessageContainerView::operator-=, factors_messages.hxx:495-508)
    const bool own_is_left = role == 0;
    const double s_left = by_right ? +1.0 : -1.0, s_right = -s_left;
    if (own_is_left) { for (int i = c.first(); i < len; i += C::STRIDE) c.own(i) += s_left * c.dl(i); }
    else { for (int i = c.first(); i < len; i += C::STRIDE) st_dual<A>(peer + i, ld_dual<A>(peer + i) + s_left * c.dl(i)); }
    if (code == OP_UP) {
      if (own_is_left) { double* m = peer + (side == 0 ? 0 : op.pd0); for (int i = c.first(); i < len; i += C::STRIDE) st_dual<A>(m + i, ld_dual<A>(m + i) + s_right * c.dl(i)); }
      else { const int o = side == 0 ? 0 : rec.d0; for (int i = c.first(); i < len; i += C::STRIDE) c.own(o + i) += s_right * c.dl(i); }
    } else if (code == OP_LABELING) {
      const int32_t* tab = tabs + op.peer_const;
      const int nl = op.pd1;
      if (own_is_left) { for (int r = c.first(); r < op.pd0; r += C::STRIDE) if (tab[r] < nl) st_dual<A>(peer + r, ld_dual<A>(peer + r) + s_right * c.dl(tab[r])); }
      else { for (int r = c.first(); r < rec.d0; r += C::STRIDE) if (tab[r] < nl) c.own(r) += s_right * c.dl(tab[r]); }
    } else {
      if (own_is_left) { for (int i = c.first(); i < len; i += C::STRIDE) st_dual<A>(peer + i, ld_dual<A>(peer + i) + s_right * c.dl(i)); }
      else { for (int i = c.first(); i < len; i += C::STRIDE) c.own(i) += s_right * c.dl(i); }
    }
    C::sync();
  };
  // The device op behind LPMP_MF_IMPROVEMENT (send_message_to_{left,right}_improvement of the message op, reference
  // factors_messages.hxx:734-747, :795-808): the exact change of LowerBound(left) + LowerBound(right) a weight-1 send
  // of this message from the factor's state after its receives would cause.  Nothing is written.
  auto improvement = [&](const Op& op) -> double {
    const int code = op.info & 15, role = (op.info >> 4) & 1, side = (op.info >> 5) & 1, pkind = (op.info >> 8) & 15;
    const double* peer = dual + op.peer_dual;
    const int len = op.len;
    const bool by_right = role == 1, own_is_left = role == 0;
    const double s_left = by_right ? +1.0 : -1.0, s_right = -s_left;
    compute_delta(op, false, true, 1.0);
    const int32_t* tab = code == OP_LABELING ? tabs + op.peer_const : nullptr;
    const int nl = op.pd1;
    const int own_io = (rec.kind_flags >> 4) & LPMP_FF_IMPLICIT_ORIGIN, peer_io = (op.info >> 7) & 1;
    double before, after;
    if (own_is_left) {          // left = this factor (vector), right = peer
      const double lb_l = vec_lb_through(c, on, [&](int i) { return c.own(i); }, own_io);
      const double la_l = vec_lb_through(c, on, [&](int i) { return i < len ? c.own(i) + s_left * c.dl(i) : c.own(i); }, own_io);
      double lb_r, la_r;
      if (code == OP_UP) {
        const int o = side == 0 ? 0 : op.pd0;
        lb_r = pw_lb_through(c, cdata, op.peer_const, pkind, op.pd0, op.pd1, [&](int j) { return ld_dual<A>(peer + j); }, t32);
        la_r = pw_lb_through(c, cdata, op.peer_const, pkind, op.pd0, op.pd1, [&](int j) { return (j >= o && j < o + len) ? ld_dual<A>(peer + j) + s_right * c.dl(j - o) : ld_dual<A>(peer + j); }, t32);
      } else if (code == OP_LABELING) {
        lb_r = vec_lb_through(c, op.pd0, [&](int j) { return ld_dual<A>(peer + j); }, peer_io);
        la_r = vec_lb_through(c, op.pd0, [&](int j) { return tab[j] < nl ? ld_dual<A>(peer + j) + s_right * c.dl(tab[j]) : ld_dual<A>(peer + j); }, peer_io);
      } else {
        lb_r = vec_lb_through(c, op.pd0, [&](int j) { return ld_dual<A>(peer + j); }, peer_io);
        la_r = vec_lb_through(c, op.pd0, [&](int j) { return ld_dual<A>(peer + j) + s_right * c.dl(j); }, peer_io);
      }
      before = lb_l + lb_r; after = la_l + la_r;
    } else {                    // left = peer (vector), right = this factor
      const double lb_l = vec_lb_through(c, op.pd0, [&](int i) { return ld_dual<A>(peer + i); }, peer_io);
      const double la_l = vec_lb_through(c, op.pd0, [&](int i) { return i < len ? ld_dual<A>(peer + i) + s_left * c.dl(i) : ld_dual<A>(peer + i); }, peer_io);
      double lb_r, la_r;
      if (code == OP_UP) {
        const int o = side == 0 ? 0 : rec.d0;
        lb_r = pw_lb_through(c, cdata, rec.const_off, okind, rec.d0, rec.d1, [&](int j) { return c.own(j); }, t32);
        la_r = pw_lb_through(c, cdata, rec.const_off, okind, rec.d0, rec.d1, [&](int j) { return (j >= o && j < o + len) ? c.own(j) + s_right * c.dl(j - o) : c.own(j); }, t32);
      } else if (code == OP_LABELING) {
        lb_r = vec_lb_through(c, on, [&](int j) { return c.own(j); }, own_io);
        la_r = vec_lb_through(c, on, [&](int j) { return tab[j] < nl ? c.own(j) + s_right * c.dl(tab[j]) : c.own(j); }, own_io);
      } else {
        lb_r = vec_lb_through(c, on, [&](int j) { return c.own(j); }, own_io);
        la_r = vec_lb_through(c, on, [&](int j) { return c.own(j) + s_right * c.dl(j); }, own_io);
      }
      before = lb_l + lb_r; after = la_l + la_r;
    }
    C::sync();
    return fabs(after - before);
  };
  // MaximizePotentialAndComputePrimal between the receives and the sends (vector factors of a COMPUTE_PRIMAL type)
  auto round_label = [&]() {
    if (!((flags & SWEEP_PRIMAL) && (rec.kind_flags & UPD_PRIMAL))) return;
    if (okind != LPMP_F_VECTOR) {
      // a pairwise factor that rounds itself (engine.cpp, ensure_primal): a side is given when its unary holds a
      // label (else when the factor's own slot does: a side without a unary), the free sides take the first minimiser
      // of T[a][b] + m1[a] + m2[b] in row-major order; the unaries of the filled sides are labelled
      if (!pw_unary) return;
      const int d0 = rec.d0, d1 = rec.d1;
      int32_t* pr = primal + 2 * (int64_t)rec.factor;
      const int u0 = pw_unary[2 * (int64_t)rec.factor], u1 = pw_unary[2 * (int64_t)rec.factor + 1];
      int x0 = u0 >= 0 ? primal[2 * (int64_t)u0] : pr[0], x1 = u1 >= 0 ? primal[2 * (int64_t)u1] : pr[1];
      const bool free0 = x0 >= d0, free1 = x1 >= d1;
      if (free0 || free1) {
        const int a0 = free0 ? 0 : x0, na = free0 ? d0 : 1, b0 = free1 ? 0 : x1, nb = free1 ? d1 : 1;
        double bv = LPMP_INF; int bi = 0x7fffffff;
        for (int i = c.first(); i < na * nb; i += C::STRIDE) {
          const int a = a0 + i / nb, b = b0 + i % nb;
          const double v = pw_cost(cdata, rec.const_off, okind, d1, a, b, t32) + c.own(a) + c.own(d0 + b);
          if (bi == 0x7fffffff || v < bv) { bv = v; bi = i; }
        }
        const double mn = C::gmin(bv);
        const int cand = C::gmin((bi != 0x7fffffff && bv == mn) ? bi : 0x7fffffff);
        x0 = a0 + cand / nb; x1 = b0 + cand % nb;
      }
      if (c.leader()) {
        pr[0] = x0; pr[1] = x1;
        if (free0 && u0 >= 0) primal[2 * (int64_t)u0] = x0;
        if (free1 && u1 >= 0) primal[2 * (int64_t)u1] = x1;
      }
      return;
    }
    double bv = LPMP_INF; int bi = 0x7fffffff;
    for (int i = c.first(); i < on; i += C::STRIDE) { const double v = c.own(i); if (bi == 0x7fffffff || v < bv) { bv = v; bi = i; } }
    const double mn = C::gmin(bv);
    const int cand = C::gmin((bi != 0x7fffffff && bv == mn) ? bi : 0x7fffffff);
    if (c.leader()) store_label(primal, rec.factor, on, cand);
  };
  Op nxt{};
  if (n_ops > 0) nxt = ops[rec.op_begin];
  for (int k = 0; k < n_ops; ++k) {
    if (k == rec.n_recv) {   // state after the receives: what every shared send is computed from
      if constexpr (G == 1 && A == ACC_WG) level_stamp(2);
      round_label();
      for (int i = c.first(); i < on; i += C::STRIDE) c.snap(i) = c.own(i);
      C::sync();
    }
    if (k == rec.n_recv && (flags & SWEEP_ADAPTIVE)) break;   // the sends of the adaptive rule follow below
    const Op op = nxt;
    if (k + 1 < n_ops) nxt = ops[rec.op_begin + k + 1];   // requested before this op's dependent chain starts
    run_op(op, k < rec.n_recv, false, op.omega);
  }
  if (rec.n_recv == n_ops) round_label();
  if ((flags & SWEEP_ADAPTIVE) && rec.n_send > 0) {
    // send_messages_with_adaptive_weights (reference factors_messages.hxx:2860-2926, non-batch branch): the dual
    // improvement of every active message for weight 1, then adaptive_weight_rescaling (:2846-2857):
    // w = omega / 2 + omega_sum / 2 * improvement / improvement_sum if that sum is positive, else the improvements
    // themselves (all 0: nothing is sent); then SendMessages(w) from the state after the receives.
    // (inactive entries have weight and improvement 0: they change neither sum)
    for (int k = 0; k < rec.n_send; ++k) {
      const Op op = ops[rec.op_begin + rec.n_recv + k];
      const double v = (op.info & OP_HAS_IMPROVEMENT) ? improvement(op) : 0.0;
      if (c.leader()) c.imp(k) = v;
    }
    C::sync();
    double isum = 0.0, osum = 0.0;
    for (int k = 0; k < rec.n_send; ++k) { isum += c.imp(k); osum += ops[rec.op_begin + rec.n_recv + k].omega; }
    if (isum > 0) {
      for (int k = 0; k < rec.n_send; ++k) {
        const Op op = ops[rec.op_begin + rec.n_recv + k];
        const double w = 0.5 * op.omega + 0.5 * osum * c.imp(k) / isum;
        if (w != 0.0) run_op(op, false, false, w);
      }
    }
  }
  if (flags & SWEEP_RESIDUAL) {   // reference send_messages_residual, factors_messages.hxx:2960-3007
    double residual = 0.0;
    for (int k = rec.n_recv; k < n_ops; ++k) {
      const Op op = ops[rec.op_begin + k];
      residual += op.omega;
      run_op(op, false, true, residual);
    }
  }
  if constexpr (G == 1 && A == ACC_WG) level_stamp(3);
  if (c.leader()) st_lb<A>(lb + rec.factor, LPMP_NAN);
  for (int i = c.first(); i < on; i += C::STRIDE) st_dual<A>(own_g + i, c.own(i));
}

template <int G>
__global__ void __launch_bounds__(GenCtx<G>::THREADS)
sweep_generic_kernel(const UpdRec* __restrict__ recs, const Op* __restrict__ ops, double* __restrict__ dual,
                     const double* __restrict__ cdata, const int32_t* __restrict__ tabs, double* __restrict__ lb,
                     int32_t* __restrict__ primal, const int32_t* __restrict__ pw_unary, int64_t first, int64_t count, int flags) {
  generic_body<G, ACC_PLAIN>(recs, ops, dual, cdata, tabs, lb, primal, pw_unary, first, count, flags, (int64_t)blockIdx.x);
}

// -------------------------------------------------------------------------------------------------
// Dense fast path: unary simplex factor with L labels whose active messages all go to dense L x L
// pairwise factors.  G lanes per factor; each lane keeps NL double2 of the table in registers, loaded
// as one coalesced 16-B-per-lane stream (2G doubles per load step = RPL rows).
//   lane g: column pair c2 = g % (L/2) (columns 2*c2, 2*c2+1), row-in-step rl = g / (L/2)
//   element of load step i: row = i*RPL + rl
// side 0 (own label = row a):    q[a] = min_b T[a][b] + m2[b]  -> reduce over the L/2 lanes of a row
// side 1 (own label = column b): q[b] = min_a T[a][b] + m1[a]  -> local over steps, reduce over the RPL row-lanes
// Vectors (theta, m1, m2, delta) live one element per lane (lane g < L) and are transposed through LDS.
// Packed for latency:
//   * the factor's record and all its ops arrive as ONE coalesced packet (no rec -> ops dependent hop);
//   * the tables of up to KMAX receives and the target vectors of up to 4 sends are requested before
//     anything is reduced, so a factor's HBM round trips overlap instead of chaining
//     (what bounds the row-major order, where a level holds only <= min(H,W) factors).
// -------------------------------------------------------------------------------------------------
template <int L> struct DenseCfg;
template <> struct DenseCfg<32> { static constexpr int G = 64; };
template <> struct DenseCfg<16> { static constexpr int G = 16; };
template <> struct DenseCfg<8>  { static constexpr int G = 8; };
template <> struct DenseCfg<4>  { static constexpr int G = 4; };

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef float float2_t __attribute__((ext_vector_type(2)));
typedef float float4_t __attribute__((ext_vector_type(4)));

template <int G, class T> __device__ __forceinline__ T uni(T v) {
  if constexpr (G == 64 && sizeof(T) == 4) return (T)__builtin_amdgcn_readfirstlane((int)v);
  else return v;
}
template <int G> __device__ __forceinline__ int64_t uni64(int64_t v) {
  if constexpr (G == 64) {
    const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffLL));
    const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return ((int64_t)hi << 32) | (unsigned int)lo;
  } else return v;
}

// Stage one factor's record + ops in the lane group's LDS slab.
//   stride > 0: packet mode, record and ops contiguous at packets[idx * stride]   (one hop)
//   stride < 0: indirect mode, record at recs[idx], then its ops at ops[op_begin]   (two hops, any op count <= cap)
template <int G>
__device__ __forceinline__ void load_packet(double2_t* slab, const Op* __restrict__ packets, const UpdRec* __restrict__ recs,
                                            const Op* __restrict__ ops, int64_t idx, int stride, bool live, int g) {
  if (stride > 0) {
    if (live) {
      const double2_t* src = reinterpret_cast<const double2_t*>(packets + idx * stride);
      for (int p = g; p < 3 * stride; p += G) slab[p] = src[p];
    }
    wave_sync();
  } else {
    if (live) {
      const double2_t* src = reinterpret_cast<const double2_t*>(recs + idx);
      if (g < 3) slab[g] = src[g];
    }
    wave_sync();
    if (live) {
      const UpdRec* hdr = reinterpret_cast<const UpdRec*>(slab);
      const int n_ops = hdr->n_recv + hdr->n_send;
      const double2_t* src = reinterpret_cast<const double2_t*>(ops + hdr->op_begin);
      for (int p = g; p < 3 * n_ops; p += G) slab[3 + p] = src[p];
    }
    wave_sync();
  }
}

// load_packet in packet mode (stride > 0) with `between` issued while the packet is in flight: loads return in the order they were
// requested, so taking the packet does not wait for what `between` asked for
template <int G, class F>
__device__ __forceinline__ void load_packet_then(double2_t* slab, const Op* __restrict__ packets, int64_t idx, int stride, bool live, int g, F between) {
  const bool has = live && g < 3 * stride;
  const double2_t* src = reinterpret_cast<const double2_t*>(packets + (live ? idx * stride : 0));
  double2_t first = double2_t{0.0, 0.0};
  if (has) first = src[g];
  between();
  if (has) slab[g] = first;
  if (live) for (int p = g + G; p < 3 * stride; p += G) slab[p] = src[p];
  wave_sync();
}

// VAR: L is the padded width; the label count of the factor (<= L) and the dims of each peer table (d0 x d1, both
// <= L, the own side's equal to the label count) are read at run time, lanes beyond them carry +inf / 0
// NT: streaming policy of the table loads.  A: access policy of the duals.  CHAIN: called from the chain executor with a
// ticket: everything constant is requested first, then the ticket's predecessors are awaited, then the duals are read.
// SHARED (the shared classes, VAR form only): every peer is a SHARED pairwise factor; its table is not fetched but read from
// the LDS slots the workgroup staged and multiplied by the peer's scale, piece by piece, where the dense form uses the registers
// it loaded.  sh_lds: per table TWO slots of L x L doubles, row stride L — V and its transpose — with NaN beyond the table's
// dims (fmin drops a NaN operand, whatever the sign of the scale; a lane whose whole row or column is padding holds a label
// the factor does not have and is never read); sh_toff[q] = offset of table q relative to cdata, n_sh tables.  A receive on
// side 0 (own label = row of V) reduces the TRANSPOSE with the column form of side 1: the lane accumulates its two columns over
// the steps and the row-lanes meet in two shuffles, instead of a DPP row reduction per step — min is exact, so q is the same
// number either way; at 32 labels that is 110 instead of 270 FP64 instructions per receive, and the pass is bound by them.
// TAB32 (SWEEP_TAB32; engine.cpp, table precision): the dense tables are stored as floats and widened where they are added —
// every dual, every sum and every minimum stays a double, so the result is the f64 body's on the widened tables bit for bit.
// The exact classes keep the 16-byte load per lane: a lane holds PER = 4 consecutive columns (a float4) of NL rows, side 0
// takes the minimum over its four columns and then over the CL = L / 4 lanes of a row, side 1 keeps four column accumulators;
// the run-time-dims classes keep the two-column mapping and load element by element.
template <int L, int KMAX, bool VAR, bool NT, int A, bool CHAIN, bool MBOX = false, bool SHARED = false, bool TAB32 = false>
__device__ __forceinline__ void dense_pk_body(const Op* __restrict__ packets, const UpdRec* __restrict__ recs, const Op* __restrict__ ops,
                                              double* __restrict__ dual, const double* __restrict__ cdata, double* __restrict__ lb,
                                              int32_t* __restrict__ primal, int64_t count, int stride, int flags, int64_t block,
                                              const ChainArgs* ca, int ticket, double* __restrict__ lbh = nullptr, int hmode = 0,
                                              unsigned long long* __restrict__ mbox = nullptr, int n_deps = -1,
                                              const double* sh_lds = nullptr, const int64_t* sh_toff = nullptr, int n_sh = 0) {
  static_assert(!SHARED || (VAR && !CHAIN && !MBOX), "the shared classes: run-time dims, plain launches");
  static_assert(!(SHARED && TAB32), "shared tables stay doubles");
  static_assert(!CHAIN || A == ACC_COH, "chain bodies hand results over through relaxed agent-scope flags: every dual access must be an agent-scope (sc1) access");
  static_assert(MAILBOX_SENDS >= 1 && MAILBOX_SENDS <= 4, "plan.hpp: the sends whose fields are held in registers (KS)");
  static_assert(!MBOX || CHAIN, "the mailbox belongs to the chain executor");   // (an instantiation of its own: the joined passes of the headline grid lost 8 % with the mailbox fields in their registers)
  constexpr int G = DenseCfg<L>::G;
  constexpr int PER = (TAB32 && !VAR) ? 4 : 2;   // table elements per lane and load step
  constexpr int CL = L / PER, RPL = PER * G / L, NL = L / RPL, GPB = 256 / G;
  using TabT = std::conditional_t<PER == 4, float4_t, double2_t>;
  constexpr int KS = MBOX ? MAILBOX_SENDS : 4;   // sends whose target vectors are prefetched / forwarded
  constexpr int NFW = MBOX ? MAILBOX_SENDS : 4;  // receives whose result can be forwarded in registers (plan.cpp: hints of mailbox chains stay below)
  constexpr int PIECES = 3 * (1 + (SHARED ? pk_indirect_cap(L) : pk_dense_cap(L)));      // 16-B pieces of the largest packet / op list
  __shared__ double2_t lds_pk[GPB][PIECES];
  __shared__ double lds_mo[GPB][L];
  __shared__ double lds_q[GPB][L];
  const int grp = threadIdx.x / G, g = threadIdx.x % G;
  const int64_t idx = block * GPB + grp;
  const bool live = idx < count;
  const int c2 = g % CL, rl = g / CL;
  load_packet<G>(lds_pk[grp], packets, recs, ops, idx, stride, live, g);
  const UpdRec* hdr = reinterpret_cast<const UpdRec*>(&lds_pk[grp][0]);
  const Op* lop = reinterpret_cast<const Op*>(&lds_pk[grp][3]);
  const int n_recv = live ? uni<G>((int)hdr->n_recv) : 0;
  const int n_send = live ? uni<G>((int)hdr->n_send) : 0;
  const bool preload_ok = live && (uni<G>(hdr->kind_flags) & UPD_PRELOAD_OK) != 0;
  double* own_g = dual + (live ? uni64<G>(hdr->dual_off) : 0);
  const int Lr = VAR ? (live ? uni<G>(hdr->d0) : 0) : L;      // label count of this factor
  const bool vl = live && g < Lr;
  double theta = 0.0;
  double sm[KS];                                 // target vectors of the first KS sends
#pragma unroll
  for (int k = 0; k < KS; ++k) sm[k] = 0.0;
  // chain executor: the fields of the first KS send ops, read from the LDS packet ONCE, before the receives write to
  // LDS — otherwise every field is re-read after those writes, one dependent LDS round trip each on the critical path
  // of a dependent level (0.64 us for two sends, tools/chain_trace.py)
  [[maybe_unused]] double* s_ms[KS]; [[maybe_unused]] double s_om[KS]; [[maybe_unused]] int s_fw[KS], s_peer[KS];
  [[maybe_unused]] unsigned long long* s_box[KS];   // mailbox row the send's vector also goes to (plan.hpp, OP_MAILBOX), or nullptr
  if constexpr (CHAIN) {
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      s_ms[k] = dual; s_om[k] = 0.0; s_fw[k] = 0; s_peer[k] = 0; s_box[k] = nullptr;
      if (k < n_send) {
        const Op& o = lop[n_recv + k];
        s_ms[k] = dual + uni64<G>(o.peer_dual) + (((uni<G>(o.info) >> 5) & 1) ? (VAR ? uni<G>(o.pd0) : L) : 0);
        s_om[k] = o.omega; s_fw[k] = uni<G>(o.pad); s_peer[k] = uni<G>(o.peer);
        if constexpr (MBOX) { if (uni<G>(o.info) & OP_MAILBOX) s_box[k] = mbox + uni64<G>(o.peer_const) * (2 * L); }
      }
    }
  }
  auto load_own_and_targets = [&]() {
    theta = vl ? ld_dual<A>(own_g + g) : 0.0;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      if (preload_ok && k < n_send && g < Lr) {
        if constexpr (CHAIN) sm[k] = ld_dual<A>(s_ms[k] + g);
        else {
          const Op& o = lop[n_recv + k];
          sm[k] = ld_dual<A>(dual + uni64<G>(o.peer_dual) + (((uni<G>(o.info) >> 5) & 1) ? (VAR ? uni<G>(o.pd0) : L) : 0) + g);
        }
      }
    }
  };
  if constexpr (!CHAIN) load_own_and_targets();
  double mnew[NFW];                              // results of receives whose store is deferred to a send
#pragma unroll
  for (int k = 0; k < NFW; ++k) mnew[k] = 0.0;
  int max_recv = n_recv;
  if (G < 64) {
#pragma unroll
    for (int m = 32; m >= G; m >>= 1) max_recv = max(max_recv, __shfl_xor(max_recv, m, 64));
  }
  bool aborted = false;
  // mailbox chains: the tracked bounds of the first chunk's peers are reduced after the sends (the next level waits for those)
  [[maybe_unused]] double late_pb[KMAX]; [[maybe_unused]] int late_peer[KMAX], late_mode[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) { late_pb[j] = LPMP_INF; late_peer[j] = -1; late_mode[j] = 0; }

  // one chunk of up to KMAX receives starting at c; FW: c is a compile-time constant and results may be forwarded;
  // FIRST (chain executor): the tables (constants) are requested, then the predecessors awaited, then the duals read
  auto chunk = [&](const int c, auto fw_tag, auto first_tag) {
    constexpr bool FW = decltype(fw_tag)::value;
    constexpr bool FIRST = decltype(first_tag)::value;
    // the tables in registers — NOT under SHARED, where t is never written: every read of a table piece goes through tab() below
    [[maybe_unused]] TabT t[KMAX][NL];
    [[maybe_unused]] const double* tsl[KMAX]; [[maybe_unused]] double tsc[KMAX];   // SHARED: the peer's table slot in LDS, its scale
    double msv[KMAX], mov[KMAX];
    int64_t pdual[KMAX];
    int side[KMAX], defer[KMAX], roff[KMAX];     // roff: offset of the own-side message vector in the peer's dual
    int dR[KMAX], dC[KMAX];
    [[maybe_unused]] const unsigned long long* box[KMAX];   // mailbox row the other side's vector is polled from, or nullptr
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {             // request everything constant first
      const bool act = c + j < n_recv;
      pdual[j] = 0; side[j] = 0; defer[j] = 0; roff[j] = 0; msv[j] = 0.0; mov[j] = 0.0; dR[j] = L; dC[j] = L; box[j] = nullptr;
      if constexpr (SHARED) { tsl[j] = sh_lds; tsc[j] = 0.0; }
      if (act) {
        const Op& o = lop[c + j];
        pdual[j] = uni64<G>(o.peer_dual);
        if constexpr (MBOX) {
          if (uni<G>(o.info) & OP_MAILBOX) { long long row; __builtin_memcpy(&row, &o.omega, 8); box[j] = mbox + uni64<G>(row) * (2 * L); }
        }
        side[j] = (uni<G>(o.info) >> 5) & 1;
        defer[j] = FW ? uni<G>(o.pad) : 0;
        const double* T = cdata + uni64<G>(o.peer_const);
        if constexpr (SHARED) {
          const int R = uni<G>(o.pd0), C = uni<G>(o.pd1);
          dR[j] = R; dC[j] = C;
          roff[j] = side[j] == 0 ? 0 : R;
          const int64_t toff = uni64<G>(__double_as_longlong(T[1]));
          int slot = -1;
          for (int q = 0; q < n_sh; ++q) if (sh_toff[q] == toff) slot = q;
          // (a table the launch did not stage would be a planning error: a NaN scale turns every dual this receive writes
          // into NaN instead of computing with another table)
          tsc[j] = slot >= 0 ? T[0] : LPMP_NAN;
          if (slot < 0) slot = 0;
          tsl[j] = sh_lds + (2 * slot + (side[j] == 0 ? 1 : 0)) * (L * L);   // side 0: the transpose
        } else
        if constexpr (VAR) {
          const int R = uni<G>(o.pd0), C = uni<G>(o.pd1);
          dR[j] = R; dC[j] = C;
          roff[j] = side[j] == 0 ? 0 : R;
          if (((uni<G>(o.info) >> 8) & 15) == LPMP_F_PAIRWISE_POTTS) {
            // a Potts neighbour among dense ones: its table diff * [a != b] is made up in registers
            const double diff = T[0];
#pragma unroll
            for (int i = 0; i < NL; ++i) {
              const int row = i * RPL + rl;
              t[j][i].x = (row < R && 2 * c2 < C) ? (row == 2 * c2 ? 0.0 : diff) : LPMP_INF;
              t[j][i].y = (row < R && 2 * c2 + 1 < C) ? (row == 2 * c2 + 1 ? 0.0 : diff) : LPMP_INF;
            }
          } else if constexpr (TAB32) {
#pragma unroll
            for (int i = 0; i < NL; ++i) {
              const int row = i * RPL + rl;
              const float* Tr = reinterpret_cast<const float*>(T) + (int64_t)row * C + 2 * c2;
              t[j][i].x = (row < R && 2 * c2 < C) ? (double)ld_stream<NT>(Tr) : LPMP_INF;
              t[j][i].y = (row < R && 2 * c2 + 1 < C) ? (double)ld_stream<NT>(Tr + 1) : LPMP_INF;
            }
          } else {
#pragma unroll
            for (int i = 0; i < NL; ++i) {
              const int row = i * RPL + rl;
              const double* Tr = T + (int64_t)row * C + 2 * c2;
              t[j][i].x = (row < R && 2 * c2 < C) ? ld_stream<NT>(Tr) : LPMP_INF;
              t[j][i].y = (row < R && 2 * c2 + 1 < C) ? ld_stream<NT>(Tr + 1) : LPMP_INF;
            }
          }
        } else if constexpr (PER == 4) {
          roff[j] = side[j] == 0 ? 0 : L;
          // consecutive lanes take consecutive 16-byte pieces: floats [4 (i G + g), + 4) = row i RPL + rl, columns 4 c2 ... 4 c2 + 3
#pragma unroll
          for (int i = 0; i < NL; ++i) t[j][i] = ld_stream<NT>(reinterpret_cast<const float4_t*>(T) + (int64_t)i * G + g);
        } else {
          roff[j] = side[j] == 0 ? 0 : L;
#pragma unroll
          for (int i = 0; i < NL; ++i) t[j][i] = ld_stream<NT>(reinterpret_cast<const double2_t*>(T + (int64_t)i * 2 * G + 2 * g));
        }
      } else if constexpr (PER == 4) {
#pragma unroll
        for (int i = 0; i < NL; ++i) t[j][i] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
      } else if constexpr (!SHARED) {
#pragma unroll
        for (int i = 0; i < NL; ++i) t[j][i] = double2_t{0.0, 0.0};
      }
    }
    // piece i of receive j's table as the lane holds it: registers, or (SHARED) one 16-byte LDS read of the staged table times
    // the peer's scale — consecutive lanes read consecutive 16-byte pieces (i * 2G + 2g doubles into the slot: conflict free)
    [[maybe_unused]] auto tab = [&](const int j, const int i) -> double2_t {
      if constexpr (PER == 4) return double2_t{0.0, 0.0};   // (the float4 form reads t directly, below)
      else if constexpr (SHARED) {
        const double2_t v = *reinterpret_cast<const double2_t*>(tsl[j] + i * 2 * G + 2 * g);
        return double2_t{tsc[j] * v.x, tsc[j] * v.y};
      } else return t[j][i];
    };
    if constexpr (CHAIN && FIRST) {              // the tables are in flight while the predecessors finish
      if (MBOX && n_deps == 0) chain_stamp(*ca, ticket, 1);   // (chain_loop_ahead knows: nothing to wait for, no barrier)
      else aborted = !chain_wait(*ca, ticket);
      load_own_and_targets();
    }
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {             // then the message vectors of these receives
      if (c + j < n_recv) {
        if constexpr (VAR) {
          if (g < Lr) msv[j] = ld_dual<A>(dual + pdual[j] + roff[j] + g);
          if (!(MBOX && box[j]) && g < (side[j] == 0 ? dC[j] : dR[j])) mov[j] = ld_dual<A>(dual + pdual[j] + (side[j] == 0 ? dR[j] : 0) + g);
        } else if (g < L) {
          msv[j] = ld_dual<A>(dual + pdual[j] + (side[j] == 0 ? 0 : L) + g);
          if (!(MBOX && box[j])) mov[j] = ld_dual<A>(dual + pdual[j] + (side[j] == 0 ? L : 0) + g);
        }
      }
    }
    if constexpr (MBOX) {                        // ... and, with everything else in flight, the vectors that come by mailbox
#pragma unroll
      for (int j = 0; j < KMAX; ++j)
        if (c + j < n_recv && box[j] && g < (VAR ? (side[j] == 0 ? dC[j] : dR[j]) : L)) mov[j] = mailbox_take(*ca, box[j] + 2 * g, aborted);
    }
    if constexpr (CHAIN && FIRST) {
      // Loads and stores share one counter on this ISA and may complete out of order with respect to each other, so a
      // wait for an older load that the compiler places after a store drains that store too — a round trip to memory
      // for a write-through store, three or four times per record (measured: 4.3 us of body per dependent level,
      // tools/chain_trace.py).  Every dual this record will read is therefore awaited HERE, before its first store.
      asm volatile("" :: "v"(theta));
#pragma unroll
      for (int k = 0; k < KS; ++k) asm volatile("" :: "v"(sm[k]));
#pragma unroll
      for (int j = 0; j < KMAX; ++j) { asm volatile("" :: "v"(msv[j])); asm volatile("" :: "v"(mov[j])); }
      chain_stamp(*ca, ticket, 4);               // duals landed
    }
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {             // then reduce, in message order
      if (c + j >= max_recv) break;
      const bool act = c + j < n_recv;
      if (g < L) lds_mo[grp][g] = mov[j];
      wave_sync();
      if constexpr (PER == 4) {
        if (side[j] == 0) {
          const double2_t ma = *reinterpret_cast<const double2_t*>(&lds_mo[grp][4 * c2]);
          const double2_t mb = *reinterpret_cast<const double2_t*>(&lds_mo[grp][4 * c2 + 2]);
#pragma unroll
          for (int i = 0; i < NL; ++i) {
            const float4_t tv = t[j][i];
            double v = fmin(fmin((double)tv.x + ma.x, (double)tv.y + ma.y), fmin((double)tv.z + mb.x, (double)tv.w + mb.y));
            if constexpr (CL > 1) v = row_allreduce_min<CL>(v);
            if (c2 == 0) lds_q[grp][i * RPL + rl] = v;
          }
        } else {
          double v0 = LPMP_INF, v1 = LPMP_INF, v2 = LPMP_INF, v3 = LPMP_INF;
#pragma unroll
          for (int i = 0; i < NL; ++i) {
            const double m1v = lds_mo[grp][i * RPL + rl];
            const float4_t tv = t[j][i];
            v0 = fmin(v0, (double)tv.x + m1v); v1 = fmin(v1, (double)tv.y + m1v);
            v2 = fmin(v2, (double)tv.z + m1v); v3 = fmin(v3, (double)tv.w + m1v);
          }
#pragma unroll
          for (int m = G / 2; m >= CL; m >>= 1) {
            v0 = fmin(v0, shfl_xor_f64(v0, m)); v1 = fmin(v1, shfl_xor_f64(v1, m));
            v2 = fmin(v2, shfl_xor_f64(v2, m)); v3 = fmin(v3, shfl_xor_f64(v3, m));
          }
          if (rl == 0) { lds_q[grp][4 * c2] = v0; lds_q[grp][4 * c2 + 1] = v1; lds_q[grp][4 * c2 + 2] = v2; lds_q[grp][4 * c2 + 3] = v3; }
        }
      } else
      if (!SHARED && side[j] == 0) {
        const double2_t mv = *reinterpret_cast<const double2_t*>(&lds_mo[grp][2 * c2]);
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          const double2_t tv = tab(j, i);
          double v = fmin(tv.x + mv.x, tv.y + mv.y);
          v = row_allreduce_min<CL>(v);
          if (c2 == 0) lds_q[grp][i * RPL + rl] = v;
        }
      } else {
        double vx = LPMP_INF, vy = LPMP_INF;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          const double m1v = lds_mo[grp][i * RPL + rl];
          const double2_t tv = tab(j, i);
          vx = fmin(vx, tv.x + m1v);
          vy = fmin(vy, tv.y + m1v);
        }
#pragma unroll
        for (int m = G / 2; m >= CL; m >>= 1) { vx = fmin(vx, shfl_xor_f64(vx, m)); vy = fmin(vy, shfl_xor_f64(vy, m)); }
        if (rl == 0) { lds_q[grp][2 * c2] = vx; lds_q[grp][2 * c2 + 1] = vy; }
      }
      wave_sync();
      double pb = LPMP_INF;                       // peer's bound after this receive
      if (act && g < Lr) {
        const double qv = lds_q[grp][g];
        const double delta = msv[j] + qv;
        theta += delta;
        const double mn = msv[j] - delta;
        pb = mn + qv;
        bool stored = false;
        if constexpr (FW) {
          if (defer[j]) {                        // c + j < NFW by construction on the host
#pragma unroll
            for (int q = 0; q < NFW; ++q) if (q == c + j) mnew[q] = mn;
            stored = true;
          }
        }
        if (!stored) st_dual<A>(dual + pdual[j] + roff[j] + g, mn);
      }
      {
        const bool track = !(FW && defer[j]);     // a deferred receive is followed by a send that dirties the peer
        const bool hist = CHAIN && hmode == HIST_MID;   // ... but its bound at the seam between two passes is this one
        if constexpr (MBOX && FIRST) {
          late_pb[j] = pb; late_peer[j] = act ? uni<G>(lop[c + j].peer) : -1; late_mode[j] = track ? 1 : 0;
        } else
        if (track || hist) {
          pb = vec_min<G, L>(pb);
          if (act && g == 0) {
            const int peer = uni<G>(lop[c + j].peer);
            if (track) st_lb<A>(lb + peer, pb);
            if (hist) st_lb<A>(lbh + peer, pb);
          }
        }
      }
      wave_sync();
    }
  };
  // the first chunks are unrolled with constant indices so that forwarded results stay in registers
  if constexpr (CHAIN) {
    chunk(0, std::true_type{}, std::true_type{});   // also waits when the workgroup's factors receive nothing
    chain_stamp(*ca, ticket, 5);                    // first receives done
  } else {
    if (max_recv > 0) chunk(0, std::true_type{}, std::false_type{});
  }
  if constexpr (KMAX < NFW) { if (max_recv > KMAX) chunk(KMAX, std::true_type{}, std::false_type{}); }
  if constexpr (2 * KMAX < NFW) { if (max_recv > 2 * KMAX) chunk(2 * KMAX, std::true_type{}, std::false_type{}); if (max_recv > 3 * KMAX) chunk(3 * KMAX, std::true_type{}, std::false_type{}); }
  for (int c = (KMAX >= NFW ? KMAX : NFW); c < max_recv; c += KMAX) chunk(c, std::false_type{}, std::false_type{});

  if (flags & SWEEP_PRIMAL) {
    const int lab = group_argmin<G, L>(theta, vl, g);
    if (live && g == 0 && (uni<G>(hdr->kind_flags) & UPD_PRIMAL)) store_label(primal, uni<G>(hdr->factor), Lr, lab);
  }
  // Bound of a pairwise peer after a SEND that follows this record's receive through the same vector (plan.cpp marks the pair:
  // Op::pad of the send = index of that receive + 1).  The receive left m_s = -q (q[a] = min_b T[a][b] + m_o[b], up to the
  // rounding of m_s - (m_s + q)), nothing else of the peer moved since, and the send adds omega * theta_snap: the peer's
  // bound min_a (m_s[a] + q[a]) is omega * min_a theta_snap[a] up to ~1e-16 of |q| per factor (sums of millions of them
  // stay below 1e-12 of the bound).  In the weight modes in which every message is received and then sent (uniform /
  // damped_uniform: the rounding iterations of MpRoundingSolver) this keeps EVERY pairwise bound tracked, and
  // LP::LowerBound after such a pass is a sum instead of a scan of all tables (C3: 0.04 instead of 3.2 ms).
  // (parked in LDS — lds_q is free once the receives are done, and only the lane that wrote it reads it back: a register
  // held across the send loops takes the 32-label chain body from 167 to 170 VGPRs, i.e. from 3 to 2 waves per SIMD)
  // Not in the mailbox bodies: there a record is a link of a latency-bound chain, and the reduction (+ 2-3 % per level,
  // measured) buys nothing — deep schedules are not what a rounding iteration's bound waits for.
  if constexpr (!MBOX) {
    const double snap_min_v = vec_min<G, L>(vl ? theta : LPMP_INF);
    if (g == 0) lds_q[grp][0] = snap_min_v;
    if constexpr (CHAIN) {   // joined passes: the factor's own bound at the seam between two passes is this minimum too
      if (hmode == HIST_MID) { if (live && g == 0) st_lb<A>(lbh + uni<G>(hdr->factor), snap_min_v); }
    }
  }
  const bool send_bounds = !MBOX && !(flags & SWEEP_RESIDUAL);   // (the residual rule adds to the sent vectors once more)
  if (vl && !aborted) {
    const double snap = theta;
    if constexpr (CHAIN) {
      // targets that could not be requested up front (a receive of this record rewrites them): all of them now, one
      // wait inside this branch — a load inside the send loop would put a wait at the loop's join that drains the
      // write-through stores of the receives on EVERY path (measured: 1 us per record, tools/chain_trace.py)
      if (!preload_ok) {
#pragma unroll
        for (int k = 0; k < KS; ++k) if (k < n_send && s_fw[k] == 0) sm[k] = ld_dual<A>(s_ms[k] + g);
#pragma unroll
        for (int k = 0; k < KS; ++k) asm volatile("" :: "v"(sm[k]));
      }
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        if (k < n_send) {
          const int fw = s_fw[k];
          const double cur = fw > 0 ? (fw == 1 ? mnew[0] : fw == 2 ? mnew[NFW > 1 ? 1 : 0] : fw == 3 ? mnew[NFW > 2 ? 2 : 0] : mnew[NFW > 3 ? 3 : 0]) : sm[k];
          const double delta = s_om[k] * snap;
          // (the residual rule below adds to the vector once more: the mailbox gets the final value there)
          if constexpr (MBOX) { if (s_box[k] && !(flags & SWEEP_RESIDUAL)) mailbox_put(s_box[k] + 2 * g, cur + delta, ca->epoch); }
          st_dual<A>(s_ms[k] + g, cur + delta);
          theta -= delta;
          // a vector that goes to the mailbox has a reader later in this launch, which sets the peer's tracked bound itself
          // — and is not ordered after THIS store, so it is left out
          if (g == 0 && !(MBOX && s_box[k])) st_lb<A>(lb + s_peer[k], fw > 0 && send_bounds ? s_om[k] * lds_q[grp][0] : LPMP_NAN);
        }
      }
      if constexpr (MBOX) chain_stamp(*ca, ticket, 6);   // first sends issued (the mailbox has them)
    } else {
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        if (k < n_send) {
          const Op& o = lop[n_recv + k];
          double* ms = dual + uni64<G>(o.peer_dual) + (((uni<G>(o.info) >> 5) & 1) ? (VAR ? uni<G>(o.pd0) : L) : 0);
          const int fw = uni<G>(o.pad);
          double cur;
          if (fw > 0) cur = fw == 1 ? mnew[0] : fw == 2 ? mnew[NFW > 1 ? 1 : 0] : fw == 3 ? mnew[NFW > 2 ? 2 : 0] : mnew[NFW > 3 ? 3 : 0];
          else cur = preload_ok ? sm[k] : ld_dual<A>(ms + g);
          const double delta = o.omega * snap;
          st_dual<A>(ms + g, cur + delta);
          theta -= delta;
          if (g == 0) st_lb<A>(lb + uni<G>(o.peer), fw > 0 && send_bounds ? o.omega * lds_q[grp][0] : LPMP_NAN);
        }
      }
    }
    // the remaining sends SC at a time: the target vectors are requested together, then updated in message order (a record
    // never sends twice into one vector: plan.cpp gives such records an op-by-op class).  One at a time, every send was a
    // dependent load -> store round trip: a variable of a random graph (C4: ten neighbours on average, up to 30) spent
    // most of its time in this loop; the first level of C4's sweep (200 000 records that only send, nine messages each) is
    // bound by exactly this chain (profiles/r03_c4c_launch_rates.txt)
    constexpr int SC = 8;
    for (int k0 = KS; k0 < n_send; k0 += SC) {
      double* msk[SC]; double cur[SC], om[SC]; int pr[SC];
#pragma unroll
      for (int q = 0; q < SC; ++q) {
        msk[q] = own_g; cur[q] = 0.0; om[q] = 0.0; pr[q] = 0;
        if (k0 + q < n_send) {
          const Op& o = lop[n_recv + k0 + q];
          msk[q] = dual + o.peer_dual + (((o.info >> 5) & 1) ? (VAR ? o.pd0 : L) : 0);
          om[q] = o.omega; pr[q] = o.peer;
          cur[q] = ld_dual<A>(msk[q] + g);
        }
      }
#pragma unroll
      for (int q = 0; q < SC; ++q) {
        if (k0 + q < n_send) {
          const double delta = om[q] * snap;
          st_dual<A>(msk[q] + g, cur[q] + delta);
          theta -= delta;
          if (g == 0) st_lb<A>(lb + pr[q], LPMP_NAN);
        }
      }
    }
    if (flags & SWEEP_RESIDUAL) {
      double residual = 0.0;
      for (int k = 0; k < n_send; ++k) {
        const Op& o = lop[n_recv + k];
        double* ms = dual + o.peer_dual + (((o.info >> 5) & 1) ? (VAR ? o.pd0 : L) : 0);
        residual += o.omega;
        const double delta = residual * theta;
        const double v = ld_dual<A>(ms + g) + delta;
        if constexpr (MBOX) { if (k < KS && (o.info & OP_MAILBOX)) mailbox_put(mbox + o.peer_const * (2 * L) + 2 * g, v, ca->epoch); }
        st_dual<A>(ms + g, v);
        theta -= delta;
      }
    }
    st_dual<A>(own_g + g, theta);
  }
  if constexpr (MBOX) {
    // (a peer this record also SENDS to ends up stale: the send's mark must be the last word, so its bound is not stored)
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      if (j >= max_recv) break;
      const double pb = vec_min<G, L>(late_pb[j]);
      if (late_peer[j] >= 0 && (late_mode[j] & 1) && g == 0) {
        bool sent = false;
        for (int k = 0; k < n_send; ++k) if (uni<G>(lop[n_recv + k].peer) == late_peer[j]) sent = true;
        if (!sent) st_lb<A>(lb + late_peer[j], pb);
      }
    }
  }
  {
    const double ob = vec_min<G, L>(vl ? theta : LPMP_INF);
    if (live && g == 0) {
      st_lb<A>(lb + uni<G>(hdr->factor), ob);
      if constexpr (CHAIN) { if (hmode == HIST_END) st_lb<A>(lbh + uni<G>(hdr->factor), ob); }
    }
  }
}

template <int L, int KMAX, bool VAR, bool NT>
__global__ void __launch_bounds__(256)
sweep_dense_pk_kernel(const Op* __restrict__ packets, const UpdRec* __restrict__ recs, const Op* __restrict__ ops,
                      double* __restrict__ dual, const double* __restrict__ cdata, double* __restrict__ lb,
                      int32_t* __restrict__ primal, int64_t count, int stride, int flags) {
  dense_pk_body<L, KMAX, VAR, NT, NT ? ACC_NT : ACC_PLAIN, false>(packets, recs, ops, dual, cdata, lb, primal, count, stride, flags,
                                                                   (int64_t)blockIdx.x, nullptr, 0);
}

// the same launch on float tables (SWEEP_TAB32): a kernel of its own, so that the f64 kernels above keep their code
template <int L, int KMAX, bool VAR, bool NT>
__global__ void __launch_bounds__(256)
sweep_dense_pk_f32_kernel(const Op* __restrict__ packets, const UpdRec* __restrict__ recs, const Op* __restrict__ ops,
                          double* __restrict__ dual, const double* __restrict__ cdata, double* __restrict__ lb,
                          int32_t* __restrict__ primal, int64_t count, int stride, int flags) {
  dense_pk_body<L, KMAX, VAR, NT, NT ? ACC_NT : ACC_PLAIN, false, false, false, true>(packets, recs, ops, dual, cdata, lb, primal, count, stride, flags,
                                                                                       (int64_t)blockIdx.x, nullptr, 0);
}

// Shared classes: unaries whose pairwise peers are all SHARED factors (cost = scale * V[a][b], V one of a handful of tables
// of the model).  A workgroup stages the launch's distinct tables in LDS ONCE (per table V and its transpose: L x L doubles each,
// row stride L, NaN beyond the table's dims) and then walks blocks of records in a grid-stride loop, so that the staging
// amortises; a receive reads its pieces of V from LDS — no table byte comes from global memory per receive.  The body is the
// dense packed body (packets / indirect records, lane mapping, send-target prefetch, tracked bounds, primal and residual rules)
// with ONE deviation: the dense form reduces a side-0 receive with a DPP row minimum per step; here both sides take the column
// form (side 0 on the staged transpose).  min is exact and order-free, so q — and with it every dual — is the same number bit for
// bit (tests/test_shared_tables_gpu.py compares with the oracle on the expansion by np.array_equal).
// LDS: the slabs of a lane group are private to its wave, so consecutive blocks of one wave need no workgroup barrier.
struct ShTabList { int32_t n; int32_t t[SHARED_MAX_TABLES]; };      // the tables of one launch (indices into the pool of ShTableDesc)
template <int L, bool NT>
__global__ void __launch_bounds__(256)
sweep_shared_pk_kernel(const Op* __restrict__ packets, const UpdRec* __restrict__ recs, const Op* __restrict__ ops,
                       double* __restrict__ dual, const double* __restrict__ cdata, double* __restrict__ lb,
                       int32_t* __restrict__ primal, int64_t count, int stride, int flags,
                       const ShTableDesc* __restrict__ desc, ShTabList list) {
  extern __shared__ __attribute__((aligned(16))) double sh_tables[];   // 2 * max(1, list.n) slots of L x L doubles: V, its transpose
  __shared__ int64_t sh_toff[SHARED_MAX_TABLES];
  const int n_sh = list.n < SHARED_MAX_TABLES ? list.n : SHARED_MAX_TABLES;
  for (int q = 0; q < n_sh; ++q) {
    const ShTableDesc d = desc[list.t[q]];
    if (threadIdx.x == 0) sh_toff[q] = d.off;
    const double* V = cdata + d.off;
    for (int x = threadIdx.x; x < L * L; x += 256) {
      const int r = x / L, c = x % L;
      const double v = (r < d.d0 && c < d.d1) ? V[r * d.d1 + c] : LPMP_NAN;
      sh_tables[(2 * q) * (L * L) + x] = v;
      sh_tables[(2 * q + 1) * (L * L) + c * L + r] = v;
    }
  }
  __syncthreads();
  constexpr int GPB = 256 / DenseCfg<L>::G;
  const int64_t n_blocks = (count + GPB - 1) / GPB;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x)
    dense_pk_body<L, 4, true, false, NT ? ACC_NT : ACC_PLAIN, false, false, true>(
        packets, recs, ops, dual, cdata, lb, primal, count, stride, flags, b, nullptr, 0, nullptr, 0, nullptr, -1, sh_tables, sh_toff, n_sh);
}

// The chain executor's launch: workgroups take tickets until none is left (kernel classes of one BODY per launch).
// The next ticket is drawn while the current one is processed, so the counter's latency is off the critical path.
template <class Body>
__device__ __forceinline__ void chain_loop(const ChainArgs& ca, const ChainLaunch* __restrict__ launches, Body body) {
  __shared__ int s_ticket[2];
  if (threadIdx.x == 0) s_ticket[0] = atomicAdd(ca.next, 1);
  __syncthreads();
  for (int it = 0;; ++it) {
    const int ticket = s_ticket[it & 1];
    if (ticket >= ca.n_tickets) break;
    if (threadIdx.x == 0) s_ticket[(it + 1) & 1] = atomicAdd(ca.next, 1);
    chain_stamp(ca, ticket, 0);                    // ticket in hand
    const TicketRef tr = chain_ticket_ref(ca, ticket);
    ChainLaunch ln = launches[ca.tk_launch[tr.idx] + tr.copy * ca.per_launch_shift];
    if (ln.pad & 3) {                                                  // joined passes: bound row of this copy's pass (HIST_* | row << 2)
      ln.pad += (tr.copy * ca.per_row_shift) << 2;
      if ((ln.pad >> 2) >= ca.hist_rows) ln.pad = 0;
    }
    body(ln, (int64_t)ca.tk_block[tr.idx], ticket);
    chain_publish(ca, ticket);
    __syncthreads();                               // s_ticket[(it + 1) & 1] is written, the LDS of the body is free again
  }
}
// MBOX: a chain whose launches all carry CHAIN_LAUNCH_MAILBOX (chain_plan.cpp marks every launch of such a chain)
// The same loop for mailbox chains, where a level is a couple of microseconds and what a workgroup needs before it can
// even request its records — ticket number (an atomic on the far side of the fabric), then the ticket's launch, block and
// dependency count (three arrays streamed from HBM once per launch: a miss each) — was 3.5 us of round trips in a row per
// ticket (tools/chain_trace.py: t1 - t0), more than a level.  Here the first thread draws ticket numbers TWO iterations
// ahead and fetches the fields of the next ticket while the current one is processed: all of it returns during the body and
// is put down in LDS after it.  (A workgroup runs its tickets in increasing order, so the lowest unfinished ticket of the
// launch is always one that is running: drawing ahead cannot deadlock.)  Costs registers: the joined passes of the shared dense body
// (167-171 VGPRs) have none to spare; the peer-minima form has, and takes a loop of its own (chain_loop_roles_ahead).
template <class Body>
__device__ __forceinline__ void chain_loop_ahead(const ChainArgs& ca, const ChainLaunch* __restrict__ launches, Body body) {
  __shared__ int s_tk[3][4];                       // ticket, launch, block, number of dependencies
  if (threadIdx.x == 0) {
    const int t = atomicAdd(ca.next, 1);
    s_tk[0][0] = t;
    if (t < ca.n_tickets) { s_tk[0][1] = ca.tk_launch[t]; s_tk[0][2] = ca.tk_block[t]; s_tk[0][3] = ca.dep_off[t + 1] - ca.dep_off[t]; }
    s_tk[1][0] = atomicAdd(ca.next, 1);
  }
  __syncthreads();
  for (int it = 0;; ++it) {
    const int cur = it % 3, nx1 = (it + 1) % 3, nx2 = (it + 2) % 3;
    const int ticket = s_tk[cur][0];
    if (ticket >= ca.n_tickets) break;
    int t2 = 0, f_launch = 0, f_block = 0, f_deps = 0;
    if (threadIdx.x == 0) {
      t2 = atomicAdd(ca.next, 1);
      const int t1 = s_tk[nx1][0];
      if (t1 < ca.n_tickets) { f_launch = ca.tk_launch[t1]; f_block = ca.tk_block[t1]; f_deps = ca.dep_off[t1 + 1] - ca.dep_off[t1]; }
    }
    chain_stamp(ca, ticket, 0);                    // ticket in hand
    if (ca.trace && threadIdx.x == 0) ca.trace[8 * (int64_t)ticket + 7] = (long long)blockIdx.x;   // ... by this workgroup
    const ChainLaunch ln = launches[s_tk[cur][1]];
    body(ln, (int64_t)s_tk[cur][2], ticket, s_tk[cur][3]);
    if (threadIdx.x == 0) { s_tk[nx1][1] = f_launch; s_tk[nx1][2] = f_block; s_tk[nx1][3] = f_deps; s_tk[nx2][0] = t2; }
    chain_publish(ca, ticket);
    __syncthreads();
  }
}
// (the exact 32-label body needs 167-171 VGPRs depending on small things: three waves per SIMD are asked for, so that it stays
// at the 170 that allows them — the joined passes of the headline grid lose 8 % at two)
template <int L, int KMAX, bool VAR, bool NT, bool MBOX>
__global__ void __launch_bounds__(256, !MBOX && L == 32 && !VAR ? 3 : 1)
chain_dense_pk_kernel(ChainArgs ca, const ChainLaunch* __restrict__ launches, double* __restrict__ dual,
                      const double* __restrict__ cdata, double* __restrict__ lb, int32_t* __restrict__ primal, int flags) {
  if constexpr (MBOX) {
    chain_loop_ahead(ca, launches, [&](const ChainLaunch& ln, int64_t block, int ticket, int n_deps) {
      dense_pk_body<L, KMAX, VAR, NT, ACC_COH, true, true>(ln.packets, ln.recs, ln.ops, dual, cdata, lb, primal, ln.count, ln.stride, flags, block, &ca, ticket,
                                                           nullptr, 0, ca.mailbox, n_deps);
    });
  } else {
    chain_loop(ca, launches, [&](const ChainLaunch& ln, int64_t block, int ticket) {
      const int hmode = ca.lb_hist ? (ln.pad & 3) : 0;
      dense_pk_body<L, KMAX, VAR, NT, ACC_COH, true>(ln.packets, ln.recs, ln.ops, dual, cdata, lb, primal, ln.count, ln.stride, flags, block, &ca, ticket,
                                                     hmode ? ca.lb_hist + (int64_t)(ln.pad >> 2) * ca.hist_stride : nullptr, hmode);
    });
  }
}

// float tables (SWEEP_TAB32): the exact 32-label body holds its two tables in 32 instead of 64 VGPRs and keeps the three waves
template <int L, int KMAX, bool VAR, bool NT, bool MBOX>
__global__ void __launch_bounds__(256, !MBOX && L == 32 && !VAR ? 3 : 1)
chain_dense_pk_f32_kernel(ChainArgs ca, const ChainLaunch* __restrict__ launches, double* __restrict__ dual,
                          const double* __restrict__ cdata, double* __restrict__ lb, int32_t* __restrict__ primal, int flags) {
  if constexpr (MBOX) {
    chain_loop_ahead(ca, launches, [&](const ChainLaunch& ln, int64_t block, int ticket, int n_deps) {
      dense_pk_body<L, KMAX, VAR, NT, ACC_COH, true, true, false, true>(ln.packets, ln.recs, ln.ops, dual, cdata, lb, primal, ln.count, ln.stride, flags, block,
                                                                        &ca, ticket, nullptr, 0, ca.mailbox, n_deps);
    });
  } else {
    chain_loop(ca, launches, [&](const ChainLaunch& ln, int64_t block, int ticket) {
      const int hmode = ca.lb_hist ? (ln.pad & 3) : 0;
      dense_pk_body<L, KMAX, VAR, NT, ACC_COH, true, false, false, true>(ln.packets, ln.recs, ln.ops, dual, cdata, lb, primal, ln.count, ln.stride, flags, block,
                                                                         &ca, ticket, hmode ? ca.lb_hist + (int64_t)(ln.pad >> 2) * ca.hist_stride : nullptr, hmode);
    });
  }
}

// ---- peer minima (joined passes of the exact 32-label f64 class) -----------------------------------------------
// In n joined passes H, W, (K, W)^(n-1), T every table is needed twice per pass: by the W record at one end of the edge and by
// the K / T record at the other.  The W record that has just SENT m' over an edge still holds the edge's table, and
// q'[a] = min_b (T[a][b] + m'[b]) is all the neighbour's next receive over that edge computes from the table.  In a launch whose
// steps carry roles (plan.hpp, CHAIN_LAUNCH_PQ_*; order.cpp decides per mode) the W records PUBLISH q' — 32 doubles in
// peerq[factor * 32 ...] — and the H / K / T records CONSUME it: they request no table and no m_o.  min is exact and every
// T[a][b] + m'[b] is one rounding whatever the lane layout, so q' is bit for bit what the consumer computes today.
// Bodies of their own, so that the shared dense body (and every kernel made from it) keeps its code.
// KM: tables a publishing record holds at once.  2 (shipped): 165 VGPRs, three waves per SIMD; the tables of the last two receives
// are still in registers when theta is final, those of the first two are requested again behind the sends (a second read, mostly
// on-die).  4: every table stays in registers from its receive to its publish, 227 VGPRs, two waves per SIMD — measured slower
// than the old form on the headline grid (1.54 against 1.61-1.65 G message updates per second; KM = 2: 1.78-1.79; EXPERIMENTS.md N).
// S: tables a publishing record PARKS in LDS between its receive and its publish (KM = 2 only).  0: the form above.  1 (shipped):
// a record with more than two receives writes table 0 to its wave's own 8 KiB of LDS before the second pair takes the registers and
// reads it back for the publish; of the first pair only table 1 is requested again, and not even that when the second pair has one
// member (its slot was never overwritten): 1.25 instead of 1.5 table requests per table and pass, the same registers, three waves
// per SIMD, 38 KiB of LDS per workgroup (EXPERIMENTS.md O; non-temporal last requests measured there as well: no difference).
// KM = 3 (shipped, LPMP_PQ_HOLD=3; a body of its own, dense_pq_publish3_body): three tables in registers and table 0 parked, so
// that every table is requested ONCE per table and pass.  It fits in 150 VGPRs without scratch because the record's fields stay in
// the packet in LDS and its vectors m_o / m_new / m' in LDS rows; 42 KiB of LDS per workgroup, three waves per SIMD.  Measured
// 3.78 against 4.17 ms per pass on the headline grid, 22.3 against 26.5 GB per pass on the fabric side (EXPERIMENTS.md R).
// LPMP_PQ_HOLD=2 selects <KM = 2, S = 1>, LPMP_PQ_LDS=0 <KM = 2, S = 0> whatever LPMP_PQ_HOLD says; both kept instruction for
// instruction.  PQ_KM names the two-table forms.
// SC (shipped, KM = 3 only; dense_pq_publish3_body<L, true> in chain_dense_pq_scatter_kernel): a publish on the column side of a
// table — every publish of the headline grid — reduces the rows with a reduce-scatter inside the 16-lane row instead of one DPP
// all-reduce per row: 8 cross-lane steps instead of 32, 78 instead of 152 VALU instructions per table and no canonicalising
// v_max_f64 (fmin_raw), 32 lanes store one minimum each.  The parent's launch was 0.42 VALU-busy; 3.50 against 3.78 ms per pass,
// the same 22.3 GB (EXPERIMENTS.md S).  The side-0 RECEIVE keeps the all-reduce (mixed-side models only; its table stays live).
// LPMP_PQ_SCATTER=0 launches chain_dense_pq_kernel<32, 3, 1, *>, kept instruction for instruction.
constexpr int PQ_KM = 2;
constexpr int PQ_OPS = PEER_MINIMA_MAX_OPS;                        // receives and sends of a record of such a launch (order.cpp checks)

// one record's packet and the fields both bodies read from it
struct PqRec {
  const UpdRec* hdr; const Op* lop;
  int n_recv, n_send; bool live, vl, preload_ok; double* own_g;
  double* s_ms[PQ_OPS]; double s_om[PQ_OPS]; int s_fw[PQ_OPS], s_peer[PQ_OPS];
  int64_t pdual[PQ_OPS]; int side[PQ_OPS], defer[PQ_OPS], rpeer[PQ_OPS];
};
// G: lanes per record.  64: a wave per record, the fields are wave-uniform scalars.  32 (consume records only, PQ_CG): two records
// per wave, every field a per-lane value read from the half-wave's own slab
// AH (tickets ahead): the first polls of the ticket's predecessors go out while the packet is in flight
template <int L, int G = 64, bool AH = false>
__device__ __forceinline__ void pq_load_rec(PqRec& r, double2_t* slab, const Op* __restrict__ packets, double* __restrict__ dual, int64_t idx, int64_t count,
                                            int stride, int g, const ChainArgs* ca = nullptr, int ticket = 0, PqAhead* ah = nullptr) {
  r.live = idx < count;
  if constexpr (AH) load_packet_then<G>(slab, packets, idx, stride, r.live, g, [&] { chain_poll_issue(*ca, ticket, *ah); });
  else load_packet<G>(slab, packets, nullptr, nullptr, idx, stride, r.live, g);
  r.hdr = reinterpret_cast<const UpdRec*>(&slab[0]);
  r.lop = reinterpret_cast<const Op*>(&slab[3]);
  r.n_recv = r.live ? min(uni<G>((int)r.hdr->n_recv), PQ_OPS) : 0;
  r.n_send = r.live ? min(uni<G>((int)r.hdr->n_send), PQ_OPS) : 0;
  r.preload_ok = r.live && (uni<G>(r.hdr->kind_flags) & UPD_PRELOAD_OK) != 0;
  r.own_g = dual + (r.live ? uni64<G>(r.hdr->dual_off) : 0);
  r.vl = r.live && g < L;
#pragma unroll
  for (int k = 0; k < PQ_OPS; ++k) {
    r.s_ms[k] = dual; r.s_om[k] = 0.0; r.s_fw[k] = 0; r.s_peer[k] = 0;
    if (k < r.n_send) {
      const Op& o = r.lop[r.n_recv + k];
      r.s_ms[k] = dual + uni64<G>(o.peer_dual) + (((uni<G>(o.info) >> 5) & 1) ? L : 0);
      r.s_om[k] = o.omega; r.s_fw[k] = uni<G>(o.pad); r.s_peer[k] = uni<G>(o.peer);
    }
  }
#pragma unroll
  for (int j = 0; j < PQ_OPS; ++j) {
    r.pdual[j] = 0; r.side[j] = 0; r.defer[j] = 0; r.rpeer[j] = 0;
    if (j < r.n_recv) {
      const Op& o = r.lop[j];
      r.pdual[j] = uni64<G>(o.peer_dual); r.side[j] = (uni<G>(o.info) >> 5) & 1; r.defer[j] = uni<G>(o.pad); r.rpeer[j] = uni<G>(o.peer);
    }
  }
}

// H, K, T: a receive is msv (its own side's vector) and the published q — no table, no m_o; from delta = msv + qv on, and in
// the sends, statement for statement what dense_pk_body does in a chain
// G = 64: a wave per record, four records per ticket, half of the lanes idle.  G = 32 (PQ_WIDE_RECORDS = 8 records per ticket,
// order.cpp plans the K / T / H blocks to match): a wave carries two records, which differ in live, n_recv, n_send, defer and
// preload_ok — so nothing that moves data across lanes (vec_min: DPP, shuffles) sits in a branch only one half takes: the
// reductions run for all four receives on every lane (+inf where there is none) and only the loads and stores are guarded.
// Per lane the arithmetic and the order of its statements are those of the 64-lane form.
// AH: a ticket of chain_loop_roles_ahead (its wait is chain_poll_issue / chain_wait_polled).  LIVE_SM (that loop's instantiation
// only): a send's own vector is preloaded only where the send uses it (s_fw == 0) — one that forwards a receive takes mnew instead,
// and every K / H / T send of a grid does.  Per lane the statements and the bits are unchanged.
template <int L, int G, bool AH = false, bool LIVE_SM = false>
__device__ __forceinline__ void dense_pq_consume_body(const Op* __restrict__ packets, double* __restrict__ dual, double* __restrict__ lb,
                                                      const double* __restrict__ peerq, int64_t count, int stride, int64_t block,
                                                      const ChainArgs* ca, int ticket, double* __restrict__ lbh, int hmode, PqAhead* ah = nullptr) {
  static_assert(G == 64 || (G == 32 && L == 32), "a wave or half a wave per record");
  constexpr int GPB = 256 / G, A = ACC_COH;
  __shared__ double2_t lds_pk[GPB][3 * (1 + PK_MAX_OPS)];
  unsigned tid = threadIdx.x;
  // (the 32-lane form's lane constants — group, lane, slab address — are made here, per ticket: hoisted out of the ticket loop they
  // would be live through the publishing body, which has no register to spare: 168 VGPRs and 12-16 bytes of scratch instead of 165 and 0)
  if constexpr (G == 32) asm volatile("" : "+v"(tid));
  const int grp = tid / G, g = tid % G;
  PqRec r;
  pq_load_rec<L, G, AH>(r, lds_pk[grp], packets, dual, block * GPB + grp, count, stride, g, ca, ticket, ah);
  bool aborted;
  if constexpr (AH) aborted = !chain_wait_polled(*ca, ticket, *ah);
  else aborted = !chain_wait(*ca, ticket);
  double theta = r.vl ? ld_dual<A>(r.own_g + g) : 0.0;
  double sm[PQ_OPS], msv[PQ_OPS], qv[PQ_OPS], mnew[PQ_OPS];
#pragma unroll
  for (int k = 0; k < PQ_OPS; ++k) { sm[k] = 0.0; if (r.preload_ok && k < r.n_send && g < L && (!LIVE_SM || r.s_fw[k] == 0)) sm[k] = ld_dual<A>(r.s_ms[k] + g); }
#pragma unroll
  for (int j = 0; j < PQ_OPS; ++j) {
    msv[j] = 0.0; qv[j] = 0.0; mnew[j] = 0.0;
    if (j < r.n_recv && g < L) {
      msv[j] = ld_dual<A>(dual + r.pdual[j] + (r.side[j] == 0 ? 0 : L) + g);
      // the slot was written by the W record that wrote the m' this record waits for anyway (see dense_pq_publish_body)
      qv[j] = ld_dual<A>(peerq + (int64_t)r.rpeer[j] * L + g);
    }
  }
  // every dual this record reads is awaited before its first store (see dense_pk_body)
  asm volatile("" :: "v"(theta));
#pragma unroll
  for (int k = 0; k < PQ_OPS; ++k) { asm volatile("" :: "v"(sm[k])); asm volatile("" :: "v"(msv[k])); asm volatile("" :: "v"(qv[k])); }
  chain_stamp(*ca, ticket, 4);
#pragma unroll
  for (int j = 0; j < PQ_OPS; ++j) {
    if constexpr (G == 64) { if (j >= r.n_recv) break; }
    const bool recv = G == 64 || j < r.n_recv;
    double pb = LPMP_INF;
    if (recv && g < L) {
      const double delta = msv[j] + qv[j];
      theta += delta;
      const double mn = msv[j] - delta;
      pb = mn + qv[j];
      if (r.defer[j]) mnew[j] = mn;
      else st_dual<A>(dual + r.pdual[j] + (r.side[j] == 0 ? 0 : L) + g, mn);
    }
    const bool track = !r.defer[j], hist = hmode == HIST_MID;
    if constexpr (G == 64) {
      if (track || hist) {
        pb = vec_min<G, L>(pb);
        if (g == 0) {
          if (track) st_lb<A>(lb + r.rpeer[j], pb);
          if (hist) st_lb<A>(lbh + r.rpeer[j], pb);
        }
      }
    } else {
      pb = vec_min<G, L>(pb);
      if (recv && g == 0) {
        if (track) st_lb<A>(lb + r.rpeer[j], pb);
        if (hist) st_lb<A>(lbh + r.rpeer[j], pb);
      }
    }
  }
  chain_stamp(*ca, ticket, 5);
  const double snap_min_v = vec_min<G, L>(r.vl ? theta : LPMP_INF);
  if (hmode == HIST_MID) { if (r.live && g == 0) st_lb<A>(lbh + uni<G>(r.hdr->factor), snap_min_v); }
  if (r.vl && !aborted) {
    const double snap = theta;
    if (!r.preload_ok) {
#pragma unroll
      for (int k = 0; k < PQ_OPS; ++k) if (k < r.n_send && r.s_fw[k] == 0) sm[k] = ld_dual<A>(r.s_ms[k] + g);
#pragma unroll
      for (int k = 0; k < PQ_OPS; ++k) asm volatile("" :: "v"(sm[k]));
    }
#pragma unroll
    for (int k = 0; k < PQ_OPS; ++k) {
      if (k < r.n_send) {
        const int fw = r.s_fw[k];
        const double cur = fw > 0 ? (fw == 1 ? mnew[0] : fw == 2 ? mnew[1] : fw == 3 ? mnew[2] : mnew[3]) : sm[k];
        const double delta = r.s_om[k] * snap;
        st_dual<A>(r.s_ms[k] + g, cur + delta);
        theta -= delta;
        if (g == 0) st_lb<A>(lb + r.s_peer[k], fw > 0 ? r.s_om[k] * snap_min_v : LPMP_NAN);
      }
    }
    st_dual<A>(r.own_g + g, theta);
  }
  const double ob = vec_min<G, L>(r.vl ? theta : LPMP_INF);
  if (r.live && g == 0) {
    st_lb<A>(lb + uni<G>(r.hdr->factor), ob);
    if (hmode == HIST_END) st_lb<A>(lbh + uni<G>(r.hdr->factor), ob);
  }
}

// a wave's parking area: [NL][64] double2_t in the registers' lane layout (16 B per lane, consecutive lanes consecutive); S = 0: none
template <int S, int NL>
__device__ __forceinline__ double2_t* pq_park_area(int grp) {
  if constexpr (S > 0) { __shared__ double2_t lds_park[256 / 64][NL * 64]; return lds_park[grp]; }
  else return nullptr;
}
// W: the receives and sends of dense_pk_body in a chain (every receive is deferred into its send: order.cpp), then the publish
template <int L, int KM, int S>
__device__ __forceinline__ void dense_pq_publish_body(const Op* __restrict__ packets, double* __restrict__ dual, const double* __restrict__ cdata,
                                                      double* __restrict__ lb, double* __restrict__ peerq, int64_t count, int stride, int64_t block,
                                                      const ChainArgs* ca, int ticket, double* __restrict__ lbh, int hmode) {
  static_assert(L == 32 && (KM == 2 || KM == 4), "the exact 32-label class");
  static_assert(S == 0 || (S == 1 && KM == 2), "one parked table beside two in registers");
  constexpr int G = 64, GPB = 256 / G, A = ACC_COH;
  constexpr int CL = L / 2, RPL = 2 * G / L, NL = L / RPL;
  __shared__ double2_t lds_pk[GPB][3 * (1 + PK_MAX_OPS)];
  __shared__ double lds_mo[GPB][L];
  __shared__ double lds_q[GPB][L];
  const int grp = threadIdx.x / G, g = threadIdx.x % G;
  const int c2 = g % CL, rl = g / CL;
  PqRec r;
  pq_load_rec<L>(r, lds_pk[grp], packets, dual, block * GPB + grp, count, stride, g);
  double2_t t[KM][NL];
  double2_t* const park = pq_park_area<S, NL>(grp);
  auto load_tab = [&](const int j, const int q) {   // table q into slot j
    const double* T = cdata + uni64<G>(r.lop[q].peer_const);
#pragma unroll
    for (int i = 0; i < NL; ++i) t[j][i] = ld_stream<false>(reinterpret_cast<const double2_t*>(T + (int64_t)i * 2 * G + 2 * g));
  };
  // keep: a slot without a table in this chunk keeps what it holds (S = 1: table 1 stays for the publish)
  auto load_tabs = [&](const int c, const bool keep) {
#pragma unroll
    for (int j = 0; j < KM; ++j) {
      if (c + j < r.n_recv) load_tab(j, c + j);
      else if (!keep) {
#pragma unroll
        for (int i = 0; i < NL; ++i) t[j][i] = double2_t{0.0, 0.0};
      }
    }
  };
  // lds_q[a] = min over the other side of T + lds_mo, for the side whose labels a are: 0 the table's rows, 1 its columns
  // (the two reductions of dense_pk_body)
  auto reduce = [&](const int j, const int side) {
    if (side == 0) {
      const double2_t mv = *reinterpret_cast<const double2_t*>(&lds_mo[grp][2 * c2]);
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const double2_t tv = t[j][i];
        double v = fmin(tv.x + mv.x, tv.y + mv.y);
        v = row_allreduce_min<CL>(v);
        if (c2 == 0) lds_q[grp][i * RPL + rl] = v;
      }
    } else {
      double vx = LPMP_INF, vy = LPMP_INF;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const double m1v = lds_mo[grp][i * RPL + rl];
        const double2_t tv = t[j][i];
        vx = fmin(vx, tv.x + m1v);
        vy = fmin(vy, tv.y + m1v);
      }
#pragma unroll
      for (int m = G / 2; m >= CL; m >>= 1) { vx = fmin(vx, shfl_xor_f64(vx, m)); vy = fmin(vy, shfl_xor_f64(vy, m)); }
      if (rl == 0) { lds_q[grp][2 * c2] = vx; lds_q[grp][2 * c2 + 1] = vy; }
    }
  };
  load_tabs(0, false);                           // constants first, then the predecessors, then the duals
  const bool aborted = !chain_wait(*ca, ticket);
  double theta = r.vl ? ld_dual<A>(r.own_g + g) : 0.0;
  double msv[PQ_OPS], mov[PQ_OPS], mnew[PQ_OPS];
#pragma unroll
  for (int j = 0; j < PQ_OPS; ++j) {
    msv[j] = 0.0; mov[j] = 0.0; mnew[j] = 0.0;
    if (j < r.n_recv && g < L) {
      msv[j] = ld_dual<A>(dual + r.pdual[j] + (r.side[j] == 0 ? 0 : L) + g);
      mov[j] = ld_dual<A>(dual + r.pdual[j] + (r.side[j] == 0 ? L : 0) + g);
    }
  }
  asm volatile("" :: "v"(theta));
#pragma unroll
  for (int j = 0; j < PQ_OPS; ++j) { asm volatile("" :: "v"(msv[j])); asm volatile("" :: "v"(mov[j])); }
  chain_stamp(*ca, ticket, 4);
#pragma unroll
  for (int c = 0; c < PQ_OPS; c += KM) {
    if (c >= r.n_recv) break;
    if (c > 0) {
      if constexpr (S == 1) {                    // every lane reads back only what it wrote itself: no wave_sync, no barrier
#pragma unroll
        for (int i = 0; i < NL; ++i) park[i * G + g] = t[0][i];
      }
      load_tabs(c, S == 1);
    }
#pragma unroll
    for (int j = 0; j < KM; ++j) {
      if (c + j >= r.n_recv) break;
      if (g < L) lds_mo[grp][g] = mov[c + j];
      wave_sync();
      reduce(j, r.side[c + j]);
      wave_sync();
      if (g < L) {
        const double qv = lds_q[grp][g];
        const double delta = msv[c + j] + qv;
        theta += delta;
        mnew[c + j] = msv[c + j] - delta;        // stored by the send that forwards it
      }
      wave_sync();
    }
  }
  chain_stamp(*ca, ticket, 5);
  const double snap_min_v = vec_min<G, L>(r.vl ? theta : LPMP_INF);
  double mpr[PQ_OPS];                            // the vector sent over the edge of receive j
#pragma unroll
  for (int j = 0; j < PQ_OPS; ++j) mpr[j] = 0.0;
  if (r.vl && !aborted) {
    const double snap = theta;
#pragma unroll
    for (int k = 0; k < PQ_OPS; ++k) {
      if (k < r.n_send) {
        const int fw = r.s_fw[k];
        const double cur = fw == 1 ? mnew[0] : fw == 2 ? mnew[1] : fw == 3 ? mnew[2] : mnew[3];
        const double delta = r.s_om[k] * snap;
        const double v = cur + delta;
        st_dual<A>(r.s_ms[k] + g, v);
        theta -= delta;
#pragma unroll
        for (int j = 0; j < PQ_OPS; ++j) if (fw == j + 1) mpr[j] = v;
        if (g == 0) st_lb<A>(lb + r.s_peer[k], r.s_om[k] * snap_min_v);
      }
    }
    st_dual<A>(r.own_g + g, theta);
  }
  // Publish: for every edge q' from the vector just stored and the table still (KM = 4) or again (KM = 2) in registers: the
  // reduction of the OTHER side, i.e. what the neighbour's receive would compute.  No new flag or wait: the slot's reader
  // is the record that already waits for this ticket because it reads the m' stored above, these are agent-scope stores
  // issued before chain_publish like that one, and the next W record that overwrites the slot already depends on that
  // reader (order.cpp plan_rotation_chain, kinds 2 / 3: both touch the pairwise factor).
  auto publish = [&](const int c) {
#pragma unroll
    for (int j = 0; j < KM; ++j) {
      if (c + j >= r.n_recv) break;
      const int q = c + j;
      if (g < L) lds_mo[grp][g] = q == 0 ? mpr[0] : q == 1 ? mpr[1] : q == 2 ? mpr[2] : mpr[3];
      wave_sync();
      reduce(j, 1 - r.side[q]);
      wave_sync();
      if (g < L && !aborted) st_dual<A>(peerq + (int64_t)r.rpeer[q] * L + g, lds_q[grp][g]);
      wave_sync();
    }
  };
  if constexpr (KM == 4) publish(0);
  else if constexpr (S == 1) {
    if (r.n_recv > KM) {
      publish(KM);
      if (r.n_recv == 2 * KM) load_tab(1, 1);    // the one table requested twice; with three receives slot 1 still holds it
#pragma unroll
      for (int i = 0; i < NL; ++i) t[0][i] = park[i * G + g];
    }
    publish(0);
  } else {
    if (r.n_recv > KM) { publish(KM); load_tabs(0, false); }
    publish(0);
  }
  const double ob = vec_min<G, L>(r.vl ? theta : LPMP_INF);
  if (r.live && g == 0) {
    st_lb<A>(lb + uni<G>(r.hdr->factor), ob);
    if (hmode == HIST_END) st_lb<A>(lbh + uni<G>(r.hdr->factor), ob);
  }
}

// W, KM = 3 (LPMP_PQ_HOLD=3): THREE tables in registers and one parked, so that no table is requested twice.  A record with four
// receives requests tables 0, 1, 2 before the wait; after receive 0 it parks table 0 in its wave's LDS area and requests table 3
// into that slot, behind receives 1 and 2; after the sends it publishes edge 3 from that slot, reads table 0 back and publishes
// 1, 2, 0 (the publishes write distinct peerq slots: their order is free).  With <= 3 receives nothing is parked.  96 VGPRs of
// tables leave 72 for everything else at three waves per SIMD, so what the shipped form keeps in registers for the whole record
// lives elsewhere: the record's fields stay in the packet in LDS and are made uniform where they are used (pq_load_rec holds them
// in > 40 SGPRs, and the kernel is at the SGPR cap), and the vectors m_o, then m_new, then m' of receive j share row j of lds_mv —
// the reductions read the row directly, the send picks its row by the run-time forward index instead of a select chain that keeps
// four vectors live.  Per lane the floating-point statements and their order are those of dense_pq_publish_body.
// AH: a ticket of chain_loop_roles_ahead — packet requested, first flag polls issued, packet taken, tables requested, polls looked at
template <int L, bool SC = false, bool AH = false>
__device__ __forceinline__ void dense_pq_publish3_body(const Op* __restrict__ packets, double* __restrict__ dual, const double* __restrict__ cdata,
                                                       double* __restrict__ lb, double* __restrict__ peerq, int64_t count, int stride, int64_t block,
                                                       const ChainArgs* ca, int ticket, double* __restrict__ lbh, int hmode, PqAhead* ah = nullptr) {
  static_assert(L == 32, "the exact 32-label class");
  constexpr int G = 64, GPB = 256 / G, A = ACC_COH, KM = 3;
  constexpr int CL = L / 2, RPL = 2 * G / L, NL = L / RPL;
  __shared__ double2_t lds_pk[GPB][3 * (1 + PK_MAX_OPS)];
  __shared__ double lds_mv[GPB][PQ_OPS][L];
  __shared__ double lds_q[GPB][L];
  const int grp = threadIdx.x / G, g = threadIdx.x % G;
  const int c2 = g % CL, rl = g / CL;
  const int64_t idx = block * GPB + grp;
  const bool live = idx < count;
  if constexpr (AH) load_packet_then<G>(lds_pk[grp], packets, idx, stride, live, g, [&] { chain_poll_issue(*ca, ticket, *ah); });
  else load_packet<G>(lds_pk[grp], packets, nullptr, nullptr, idx, stride, live, g);
  const UpdRec* const hdr = reinterpret_cast<const UpdRec*>(&lds_pk[grp][0]);
  const Op* const lop = reinterpret_cast<const Op*>(&lds_pk[grp][3]);
  const int n_recv = live ? min(uni<G>((int)hdr->n_recv), PQ_OPS) : 0;
  const int n_send = live ? min(uni<G>((int)hdr->n_send), PQ_OPS) : 0;
  const bool vl = live && g < L;
  auto side_of = [&](const int j) { return (uni<G>(lop[j].info) >> 5) & 1; };
  double2_t t[KM][NL];
  double2_t* const park = pq_park_area<1, NL>(grp);
  auto load_tab = [&](const int s, const int q) {   // table q into slot s
    const double2_t* T = reinterpret_cast<const double2_t*>(cdata + uni64<G>(lop[q].peer_const)) + g;
#pragma unroll
    for (int i = 0; i < NL; ++i) t[s][i] = ld_stream<false>(T + i * G);
  };
  // lds_q[a] = min over the other side of T + mo, as in dense_pq_publish_body; mo is a row of lds_mv
  auto reduce = [&](const int s, const int side, const double* mo) {
    if (side == 0) {
      const double2_t mv = *reinterpret_cast<const double2_t*>(&mo[2 * c2]);
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const double2_t tv = t[s][i];
        double v = fmin(tv.x + mv.x, tv.y + mv.y);
        v = row_allreduce_min<CL>(v);
        if (c2 == 0) lds_q[grp][i * RPL + rl] = v;
      }
    } else {
      double vx = LPMP_INF, vy = LPMP_INF;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const double m1v = mo[i * RPL + rl];
        const double2_t tv = t[s][i];
        vx = fmin(vx, tv.x + m1v);
        vy = fmin(vy, tv.y + m1v);
      }
#pragma unroll
      for (int m = G / 2; m >= CL; m >>= 1) { vx = fmin(vx, shfl_xor_f64(vx, m)); vy = fmin(vy, shfl_xor_f64(vy, m)); }
      if (rl == 0) { lds_q[grp][2 * c2] = vx; lds_q[grp][2 * c2 + 1] = vy; }
    }
  };
  // SC: the side-0 reduction of a PUBLISH as a reduce-scatter.  All eight row partials of the lane first; then three halving
  // exchanges inside the 16-lane row — a lane keeps the rows i whose bit 2, 1, 0 is bit 3, 2, 1 of its c2, so 4, 2 and 1 values
  // move — and one pairing step (lane ^ 1): 8 cross-lane steps where the all-reduce above runs 32, and lane c2 ends with the
  // minimum of row i = c2 >> 1 alone.  The even lanes store it: 32 lanes one entry each.  The slot is dead afterwards, so the
  // partials take its registers.  min is exact and every sum is the one above: the same bits.
  auto scatter = [&](const int s, const double* mo) {
    static_assert(!SC || (NL == 8 && CL == 16), "three halvings of eight rows over a 16-lane row");
    const double2_t mv = *reinterpret_cast<const double2_t*>(&mo[2 * c2]);
    double v[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const double2_t tv = t[s][i];
      v[i] = fmin(tv.x + mv.x, tv.y + mv.y);
    }
    double w[4], x[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = dpp_halve_min<0x140, 0x3>(v[k], v[4 + k]);   // row_mirror: lanes 0-7 keep rows 0-3
#pragma unroll
    for (int k = 0; k < 2; ++k) x[k] = dpp_halve_min<0x141, 0x5>(w[k], w[2 + k]);   // row_half_mirror: banks 0 and 2 keep the lower two
    const bool up = (c2 & 2) != 0;                                                  // lane ^ 2 stays inside a bank: a select
    double y = fmin_raw(up ? x[1] : x[0], dpp_mov_f64<0x4E>(up ? x[0] : x[1]));
    y = fmin_raw(y, dpp_mov_f64<0xB1>(y));                                           // lane ^ 1: the pair that holds the row's two halves
    if ((c2 & 1) == 0) lds_q[grp][(c2 >> 1) * RPL + rl] = y;
  };
#pragma unroll
  for (int j = 0; j < KM; ++j) {                   // constants first, then the predecessors, then the duals
    if (j < n_recv) load_tab(j, j);
    else {
#pragma unroll
      for (int i = 0; i < NL; ++i) t[j][i] = double2_t{0.0, 0.0};
    }
  }
  bool aborted;
  if constexpr (AH) aborted = !chain_wait_polled(*ca, ticket, *ah);
  else aborted = !chain_wait(*ca, ticket);
  double* const own_g = dual + (live ? uni64<G>(hdr->dual_off) : 0);
  double theta = vl ? ld_dual<A>(own_g + g) : 0.0;
  double msv[PQ_OPS], mov[PQ_OPS];
#pragma unroll
  for (int j = 0; j < PQ_OPS; ++j) {
    msv[j] = 0.0; mov[j] = 0.0;
    if (j < n_recv && g < L) {
      const double* pd = dual + uni64<G>(lop[j].peer_dual);
      const int sd = side_of(j);
      msv[j] = ld_dual<A>(pd + (sd == 0 ? 0 : L) + g);
      mov[j] = ld_dual<A>(pd + (sd == 0 ? L : 0) + g);
    }
  }
  asm volatile("" :: "v"(theta));
#pragma unroll
  for (int j = 0; j < PQ_OPS; ++j) { asm volatile("" :: "v"(msv[j])); asm volatile("" :: "v"(mov[j])); }
  chain_stamp(*ca, ticket, 4);
  if (g < L) {
#pragma unroll
    for (int j = 0; j < PQ_OPS; ++j) lds_mv[grp][j][g] = mov[j];
  }
  wave_sync();
  auto receive = [&](const int j, const int s) {   // row j: m_o in, m_new out (stored by the send that forwards it)
    reduce(s, side_of(j), lds_mv[grp][j]);
    wave_sync();
    if (g < L) {
      const double qv = lds_q[grp][g];
      const double delta = msv[j] + qv;
      theta += delta;
      lds_mv[grp][j][g] = msv[j] - delta;
    }
    wave_sync();
  };
  if (n_recv > 0) receive(0, 0);
  if (n_recv > KM) {                               // every lane reads back only what it wrote itself: no wave_sync, no barrier
#pragma unroll
    for (int i = 0; i < NL; ++i) park[i * G + g] = t[0][i];
    load_tab(0, KM);
  }
  if (n_recv > 1) receive(1, 1);
  if (n_recv > 2) receive(2, 2);
  if (n_recv > KM) receive(KM, 0);
  chain_stamp(*ca, ticket, 5);
  const double snap_min_v = vec_min<G, L>(vl ? theta : LPMP_INF);
  if (vl && !aborted) {
    const double snap = theta;
#pragma unroll
    for (int k = 0; k < PQ_OPS; ++k) {
      if (k < n_send) {
        const Op& o = lop[n_recv + k];
        const int fw = uni<G>(o.pad);
        double* const row = lds_mv[grp][fw >= 1 && fw < PQ_OPS ? fw - 1 : PQ_OPS - 1];
        const double om = o.omega;
        const double delta = om * snap;
        const double v = row[g] + delta;
        st_dual<A>(dual + uni64<G>(o.peer_dual) + (((uni<G>(o.info) >> 5) & 1) ? L : 0) + g, v);
        theta -= delta;
        row[g] = v;                                // m': what the publish of that edge reduces
        if (g == 0) st_lb<A>(lb + uni<G>(o.peer), om * snap_min_v);
      }
    }
    st_dual<A>(own_g + g, theta);
  }
  wave_sync();
  // Publish (see dense_pq_publish_body): the reduction of the OTHER side from the vector just stored
  auto publish = [&](const int q, const int s) {
    if constexpr (SC) {
      if (side_of(q) == 1) scatter(s, lds_mv[grp][q]);
      else reduce(s, 1, lds_mv[grp][q]);
    } else reduce(s, 1 - side_of(q), lds_mv[grp][q]);
    wave_sync();
    if (g < L && !aborted) st_dual<A>(peerq + (int64_t)uni<G>(lop[q].peer) * L + g, lds_q[grp][g]);
    wave_sync();
  };
  if (n_recv > KM) {
    publish(KM, 0);
#pragma unroll
    for (int i = 0; i < NL; ++i) t[0][i] = park[i * G + g];
  }
  if (n_recv > 1) publish(1, 1);
  if (n_recv > 2) publish(2, 2);
  if (n_recv > 0) publish(0, 0);
  const double ob = vec_min<G, L>(vl ? theta : LPMP_INF);
  if (live && g == 0) {
    st_lb<A>(lb + uni<G>(hdr->factor), ob);
    if (hmode == HIST_END) st_lb<A>(lbh + uni<G>(hdr->factor), ob);
  }
}

// chain_loop for launches whose steps carry a role in ChainLaunch::pad above the bound row
template <class Body>
__device__ __forceinline__ void chain_loop_roles(const ChainArgs& ca, const ChainLaunch* __restrict__ launches, Body body) {
  __shared__ int s_ticket[2];
  if (threadIdx.x == 0) s_ticket[0] = atomicAdd(ca.next, 1);
  __syncthreads();
  for (int it = 0;; ++it) {
    const int ticket = s_ticket[it & 1];
    if (ticket >= ca.n_tickets) break;
    if (threadIdx.x == 0) s_ticket[(it + 1) & 1] = atomicAdd(ca.next, 1);
    chain_stamp(ca, ticket, 0);
    const TicketRef tr = chain_ticket_ref(ca, ticket);
    ChainLaunch ln = launches[ca.tk_launch[tr.idx] + tr.copy * ca.per_launch_shift];
    const int role = ln.pad & CHAIN_LAUNCH_PQ_MASK;
    ln.pad &= ~CHAIN_LAUNCH_PQ_MASK;
    if (ln.pad & 3) {
      ln.pad += (tr.copy * ca.per_row_shift) << 2;
      if ((ln.pad >> 2) >= ca.hist_rows) ln.pad = 0;
    }
    body(ln, (int64_t)ca.tk_block[tr.idx], ticket, role);
    chain_publish(ca, ticket);
    __syncthreads();
  }
}
// CG: lanes per CONSUME record (dense_pq_consume_body): 64, or 32 for PQ_WIDE_RECORDS records per consume ticket
static_assert(PQ_WIDE_RECORDS == 256 / 32, "plan.hpp: records per consume ticket of the wide form");
template <int L, int KM, int S = 0, int CG = 64>
__global__ void __launch_bounds__(256, KM == 4 ? 2 : 3)
chain_dense_pq_kernel(ChainArgs ca, const ChainLaunch* __restrict__ launches, double* __restrict__ dual, const double* __restrict__ cdata,
                      double* __restrict__ lb, double* __restrict__ peerq) {
  chain_loop_roles(ca, launches, [&](const ChainLaunch& ln, int64_t block, int ticket, int role) {
    const int hmode = ca.lb_hist ? (ln.pad & 3) : 0;
    double* lbh = hmode ? ca.lb_hist + (int64_t)(ln.pad >> 2) * ca.hist_stride : nullptr;
    if (role == CHAIN_LAUNCH_PQ_PUBLISH) {
      if constexpr (KM == 3) dense_pq_publish3_body<L>(ln.packets, dual, cdata, lb, peerq, ln.count, ln.stride, block, &ca, ticket, lbh, hmode);
      else dense_pq_publish_body<L, KM, S>(ln.packets, dual, cdata, lb, peerq, ln.count, ln.stride, block, &ca, ticket, lbh, hmode);
    } else dense_pq_consume_body<L, CG>(ln.packets, dual, lb, peerq, ln.count, ln.stride, block, &ca, ticket, lbh, hmode);
  });
}

// the three-table form with the publish's row reduction as a reduce-scatter (dense_pq_publish3_body<L, true>): a kernel of its
// own, so that chain_dense_pq_kernel<32, 3, 1, *> keeps its symbols and its code (LPMP_PQ_SCATTER=0 launches those)
template <int L, int CG>
__global__ void __launch_bounds__(256, 3)
chain_dense_pq_scatter_kernel(ChainArgs ca, const ChainLaunch* __restrict__ launches, double* __restrict__ dual, const double* __restrict__ cdata,
                              double* __restrict__ lb, double* __restrict__ peerq) {
  chain_loop_roles(ca, launches, [&](const ChainLaunch& ln, int64_t block, int ticket, int role) {
    const int hmode = ca.lb_hist ? (ln.pad & 3) : 0;
    double* lbh = hmode ? ca.lb_hist + (int64_t)(ln.pad >> 2) * ca.hist_stride : nullptr;
    if (role == CHAIN_LAUNCH_PQ_PUBLISH) dense_pq_publish3_body<L, true>(ln.packets, dual, cdata, lb, peerq, ln.count, ln.stride, block, &ca, ticket, lbh, hmode);
    else dense_pq_consume_body<L, CG>(ln.packets, dual, lb, peerq, ln.count, ln.stride, block, &ca, ticket, lbh, hmode);
  });
}

// chain_loop_roles with the next ticket's descriptor fetched during the current body (the joined passes had no register for it at
// 167-171 VGPRs; the three-table form has: it costs the one VGPR of the descriptor word and the drawn number).  Ticket numbers are
// drawn exactly where chain_loop_roles draws them, one ahead, but the atomic's result stays in a register of thread 0 until the
// wait's barrier (chain_wait_polled), where wave 0 puts it down and requests that ticket's descriptor, one word per lane; the word
// lands in s_desc behind the body.  The call's launch table (ChainAhead::n_launches <= PQ_AHEAD_MAX_LAUNCHES entries) is copied to
// LDS once per workgroup, so a ticket's ChainLaunch costs no round trip either.  A ticket thus begins with everything but its
// packet in LDS.  s_desc / s_ticket [(it + 1) & 1] were last read in iteration it - 1, two barriers ago.
template <class Body>
__device__ __forceinline__ void chain_loop_roles_ahead(const ChainArgs& ca, const ChainAhead& aa, const ChainLaunch* __restrict__ launches, Body body) {
  __shared__ int s_ticket[2];
  __shared__ int s_desc[2][TICKET_DESC_WORDS];
  __shared__ int s_bad;
  __shared__ long long s_ln[PQ_AHEAD_MAX_LAUNCHES * (sizeof(ChainLaunch) / 8)];
  constexpr int LW = (int)(sizeof(ChainLaunch) / 8);
  for (int i = (int)threadIdx.x; i < aa.n_launches * LW; i += (int)blockDim.x) s_ln[i] = reinterpret_cast<const long long*>(launches)[i];
  if (threadIdx.x == 0) { s_ticket[0] = atomicAdd(ca.next, 1); s_bad = 0; }
  __syncthreads();
  {
    const int t = s_ticket[0];
    if (t < ca.n_tickets && threadIdx.x < TICKET_DESC_WORDS) s_desc[0][threadIdx.x] = aa.desc[(int64_t)chain_ticket_ref(ca, t).idx * TICKET_DESC_WORDS + threadIdx.x];
  }
  __syncthreads();
  for (int it = 0;; ++it) {
    const int ticket = s_ticket[it & 1];
    if (ticket >= ca.n_tickets) break;
    PqAhead ah;
    ah.aa = &aa; ah.next = 0; ah.word = 0;
    if (threadIdx.x == 0) ah.next = atomicAdd(ca.next, 1);
    chain_stamp(ca, ticket, 0);
    ah.desc = s_desc[it & 1]; ah.copy = chain_ticket_ref(ca, ticket).copy;
    ah.s_next = &s_ticket[(it + 1) & 1]; ah.s_bad = &s_bad;
    const long long* lw = s_ln + (ah.desc[TD_LAUNCH] + ah.copy * ca.per_launch_shift) * LW;
    ChainLaunch ln;
    ln.packets = reinterpret_cast<const Op*>(lw[0]); ln.recs = reinterpret_cast<const UpdRec*>(lw[1]); ln.ops = reinterpret_cast<const Op*>(lw[2]);
    ln.count = lw[3]; ln.stride = (int32_t)(lw[4] & 0xffffffffLL); ln.pad = (int32_t)(lw[4] >> 32);
    const int role = ln.pad & CHAIN_LAUNCH_PQ_MASK;
    ln.pad &= ~CHAIN_LAUNCH_PQ_MASK;
    if (ln.pad & 3) {
      ln.pad += (ah.copy * ca.per_row_shift) << 2;
      if ((ln.pad >> 2) >= ca.hist_rows) ln.pad = 0;
    }
    body(ln, (int64_t)ah.desc[TD_BLOCK], ticket, role, ah);
    if (threadIdx.x < TICKET_DESC_WORDS) s_desc[(it + 1) & 1][threadIdx.x] = ah.word;
    chain_publish(ca, ticket);
    if (threadIdx.x == 0) s_bad = 0;               // (every thread has read it: the publish has a barrier)
    __syncthreads();
  }
}
static_assert(sizeof(ChainLaunch) == 40 && offsetof(ChainLaunch, count) == 24 && offsetof(ChainLaunch, stride) == 32 && offsetof(ChainLaunch, pad) == 36, "chain_loop_roles_ahead reads a ChainLaunch as five 8-byte words");
// chain_dense_pq_scatter_kernel<L, 32> on that loop; LIVE_SM: dense_pq_consume_body (false: measurements, LPMP_PQ_AHEAD=2)
template <int L, int CG, bool LIVE_SM>
__global__ void __launch_bounds__(256, 3)
chain_dense_pq_ahead_kernel(ChainArgs ca, ChainAhead aa, const ChainLaunch* __restrict__ launches, double* __restrict__ dual, const double* __restrict__ cdata,
                            double* __restrict__ lb, double* __restrict__ peerq) {
  chain_loop_roles_ahead(ca, aa, launches, [&](const ChainLaunch& ln, int64_t block, int ticket, int role, PqAhead& ah) {
    const int hmode = ca.lb_hist ? (ln.pad & 3) : 0;
    double* lbh = hmode ? ca.lb_hist + (int64_t)(ln.pad >> 2) * ca.hist_stride : nullptr;
    if (role == CHAIN_LAUNCH_PQ_PUBLISH) dense_pq_publish3_body<L, true, true>(ln.packets, dual, cdata, lb, peerq, ln.count, ln.stride, block, &ca, ticket, lbh, hmode, &ah);
    else dense_pq_consume_body<L, CG, true, LIVE_SM>(ln.packets, dual, lb, peerq, ln.count, ln.stride, block, &ca, ticket, lbh, hmode, &ah);
  });
}

// the generic kernels inside the chain executor (chains of tiny factors: multicut / C5 labeling lists): nothing
// constant worth requesting ahead, so the wait comes first
static_assert(GEN_WAVES == GENERIC_BLOCK_RECORDS && 64 * SMALL_WAVES == SMALL_BLOCK_RECORDS, "plan.hpp: records per workgroup of the generic kernels");
template <int G>
__global__ void __launch_bounds__(GenCtx<G>::THREADS)
chain_generic_kernel(ChainArgs ca, const ChainLaunch* __restrict__ launches, double* __restrict__ dual, const double* __restrict__ cdata,
                     const int32_t* __restrict__ tabs, double* __restrict__ lb, int flags) {
  chain_loop(ca, launches, [&](const ChainLaunch& ln, int64_t block, int ticket) {
    if (chain_wait(ca, ticket)) generic_body<G, ACC_COH>(ln.recs, ln.ops, dual, cdata, tabs, lb, nullptr, nullptr, 0, ln.count, flags, block);
  });
}

// Level loop: a deep schedule of TINY levels of a generic class as one launch of ONE workgroup that walks the launches in
// order with a workgroup barrier in between (chain_plan.cpp decides; C5 with local triples: 11 887 levels of a dozen one-lane
// updates).  No launch per level, no flags through memory; what a level hands to the next stays in this compute unit's L2
// (stores drained before the barrier, dual loads that bypass the L1: ACC_WG).
//   G = 64 (wave per factor): the plain body.
//   G = 1 (lane per factor): LL_WAVES computing waves + one wave that touches, LEVEL_LOOP_AHEAD levels ahead, every
//   line the computing waves will need (records, op lists, match tables, own and peer duals).  Launches of
//   labeling-list records run with one lane per op (label_ops_body), the others on the generic body (one wave).
constexpr int LEVEL_LOOP_AHEAD = 8;
constexpr int LL_WAVES = 2;                        // computing waves of level_loop_kernel<1> (+ one that runs ahead)

// Labeling-list records with one LANE PER OP (chain_plan.cpp marks the launches: vector factors whose ops are all labeling
// messages with the factor on the left, at most 8 receives with distinct peers and 8 sends with distinct peers, message
// length = the factor's size).
// One record per lane runs as many op rounds as its longest receive and send lists (generic_body<1>; measured
// 9.8 + 4.3 us per level on C5 with local triples); but the receives of one record do not depend on each other —
// each delta comes from its peer alone — and neither do its sends, which all start from the snapshot.  So 8 lanes
// take one record: lane j computes op j, the deltas meet in LDS and are added to the factor's vector in op order
// (same additions, same order as the sequential form: bit-identical), two rounds — the receives, then the sends —
// instead of n_recv + n_send.
// A level of the level loop staged in LDS by the wave that runs ahead (level_loop_kernel<1>): the records, their ops and
// the match tables of their labeling messages — everything CONSTANT a level needs.  Read from the L2 they are a chain of
// three dependent round trips (launch -> record -> op -> table) in front of the one that matters (the peers' costs); of the
// ~5 round trips a level of C5's local triples took (5.4 us, 64 ms per pass) they were more than half.
constexpr int LL_RING = 4;                         // (LL_STAGE_RECS, LL_STAGE_OPS: plan.hpp)
static_assert(LL_STAGE_OPS == 8 + 8 && 4 * 64 == LL_STAGE_RECS * LL_STAGE_OPS, "one op slot per lane of the staging wave in four rounds");
// doubles of the peer an op touches: pd1 is a second dimension only for a pairwise peer (OP_UP); for a labeling message it is the
// table's n_left and the peer a vector of pd0 entries
__device__ __forceinline__ int peer_dual_size(const Op& o) { return (o.info & 15) == OP_UP ? o.pd0 + o.pd1 : o.pd0; }
struct alignas(16) StagedLevel {
  UpdRec recs[LL_STAGE_RECS];
  Op ops[LL_STAGE_RECS][LL_STAGE_OPS];
  int32_t tab[LL_STAGE_RECS][LL_STAGE_OPS][SMALL_MAXD];
  const Op* ops_base;   // the launch's op array (for the stage that copies the ops)
  int32_t count;        // records staged, or -1: this level is read from memory (not a labeling-list launch, or too large)
  int32_t pad[1];
};
template <int A, bool PAIRED, bool STAGED = false>
__device__ __forceinline__ void label_ops_body(const ChainLaunch& ln, int64_t first, double* __restrict__ dual, const int32_t* __restrict__ tabs,
                                               double* __restrict__ lb, double (*D)[8][8], double (*S)[8], const StagedLevel* st = nullptr) {
  const int lane = threadIdx.x & 63, q = lane >> 3, j = lane & 7;
  const int64_t idx = first + q;
  const bool live = idx < ln.count;
  UpdRec rec;
  if (live) { if constexpr (STAGED) rec = st->recs[idx]; else rec = ln.recs[idx]; }
  else { rec.n_recv = 0; rec.n_send = 0; rec.d0 = 0; rec.dual_off = 0; rec.op_begin = 0; rec.factor = 0; }
  const int n_recv = rec.n_recv, n_send = rec.n_send, on = rec.d0;
  double* own_g = dual + rec.dual_off;
  double theta = (live && j < on) ? ld_dual<A>(own_g + j) : 0.0;      // lane j of the group holds element j
  // one op of this lane: its record, match table and the peer's costs; entries beyond the peer's size count as no match
  auto load_op = [&](bool has, int k, Op& o, int (&tv)[SMALL_MAXD], double (&R)[SMALL_MAXD]) {
    if (has) { if constexpr (STAGED) o = st->ops[idx][k]; else o = ln.ops[rec.op_begin + k]; }
    else { o.peer_dual = 0; o.peer_const = 0; o.omega = 0.0; o.info = 0; o.pd0 = 0; o.pd1 = 0; o.peer = 0; o.len = 0; }
    const double* peer = dual + o.peer_dual;
    const int32_t* tab = tabs + o.peer_const;
#pragma unroll
    for (int r = 0; r < SMALL_MAXD; ++r) {
      const bool in = has && r < o.pd0;
      if constexpr (STAGED) tv[r] = in ? st->tab[idx][k][r] : o.pd1; else tv[r] = in ? tab[r] : o.pd1;
      R[r] = in ? ld_dual<A>(peer + r) : LPMP_INF;
    }
  };
  if constexpr (PAIRED) {
    // every message of the record is received and then sent (send j goes where receive j came from): the peer's costs
    // stay in this lane's registers between the two rounds — one load and one store per peer, no drain in between
    const bool act = live && j < n_recv;
    Op o; int tv[SMALL_MAXD]; double R[SMALL_MAXD];
    load_op(act, j, o, tv, R);
    double omega_send = 0.0;
    if (act) { if constexpr (STAGED) omega_send = st->ops[idx][n_recv + j].omega; else omega_send = ln.ops[rec.op_begin + n_recv + j].omega; }
    const int nl = o.pd1;
    if (act) {
      st_lb<A>(lb + o.peer, LPMP_NAN);
      double nt = ((o.info >> 6) & 1) ? 0.0 : LPMP_INF;
#pragma unroll
      for (int r = 0; r < SMALL_MAXD; ++r) if (tv[r] >= nl) nt = fmin(nt, R[r]);
      for (int l = 0; l < nl; ++l) {
        double v = LPMP_INF;
#pragma unroll
        for (int r = 0; r < SMALL_MAXD; ++r) if (tv[r] == l) v = fmin(v, R[r]);
        D[q][j][l] = o.omega * (v - nt);
      }
#pragma unroll
      for (int r = 0; r < SMALL_MAXD; ++r) if (r < o.pd0 && tv[r] < nl) R[r] = R[r] + -1.0 * D[q][j][tv[r]];
    }
    wave_sync();
    for (int k = 0; k < n_recv; ++k) if (j < on) theta += +1.0 * D[q][k][j];
    if (live && j < on) S[q][j] = theta;
    wave_sync();
    if (act) {
      double* peer = dual + o.peer_dual;
      for (int l = 0; l < o.len; ++l) D[q][j][l] = omega_send * S[q][l];
#pragma unroll
      for (int r = 0; r < SMALL_MAXD; ++r) if (r < o.pd0 && tv[r] < nl) st_dual<A>(peer + r, R[r] + +1.0 * D[q][j][tv[r]]);
    }
  } else {
  static_assert(!STAGED, "the staged form of the general case is label_ops_body_staged");
  Op o2; int tv2[SMALL_MAXD]; double R2[SMALL_MAXD];
  {   // round 1: the receives, lane j = receive j
    const bool recv = live && j < n_recv;
    Op o; int tv[SMALL_MAXD]; double R[SMALL_MAXD];
    load_op(recv, j, o, tv, R);
    if (recv) {
      const int nl = o.pd1;
      double* peer = dual + o.peer_dual;
      st_lb<A>(lb + o.peer, LPMP_NAN);
      double nt = ((o.info >> 6) & 1) ? 0.0 : LPMP_INF;
#pragma unroll
      for (int r = 0; r < SMALL_MAXD; ++r) if (tv[r] >= nl) nt = fmin(nt, R[r]);
      for (int l = 0; l < nl; ++l) {
        double v = LPMP_INF;
#pragma unroll
        for (int r = 0; r < SMALL_MAXD; ++r) if (tv[r] == l) v = fmin(v, R[r]);
        D[q][j][l] = o.omega * (v - nt);
      }
#pragma unroll
      for (int r = 0; r < SMALL_MAXD; ++r) if (r < o.pd0 && tv[r] < nl) st_dual<A>(peer + r, R[r] + -1.0 * D[q][j][tv[r]]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // a send of this record may go to the peer a receive has just rewritten
  wave_sync();
  for (int k = 0; k < n_recv; ++k) if (j < on) theta += +1.0 * D[q][k][j];   // own(i) += +1.0 * dl(i), receive by receive
  if (live && j < on) S[q][j] = theta;                                        // the state every send starts from
  wave_sync();
  {   // round 2: the sends, lane j = send j
    const bool send = live && j < n_send;
    load_op(send, n_recv + j, o2, tv2, R2);
    if (send) {
      const int nl = o2.pd1;
      double* peer = dual + o2.peer_dual;
      st_lb<A>(lb + o2.peer, LPMP_NAN);
      for (int l = 0; l < o2.len; ++l) D[q][j][l] = o2.omega * S[q][l];
#pragma unroll
      for (int r = 0; r < SMALL_MAXD; ++r) if (r < o2.pd0 && tv2[r] < nl) st_dual<A>(peer + r, R2[r] + +1.0 * D[q][j][tv2[r]]);
    }
  }
  }
  wave_sync();
  for (int k = 0; k < n_send; ++k) if (j < on) theta += -1.0 * D[q][k][j];   // own(i) += -1.0 * dl(i), send by send
  if (live && j == 0) st_lb<A>(lb + rec.factor, LPMP_NAN);
  if (live && j < on) st_dual<A>(own_g + j, theta);
}

// The staged form of the general (not PAIRED) case.  Records, ops and match tables come from LDS (StagedLevel), so the only
// round trip in front of the arithmetic is the peers' costs — and the sends need none of their own: a send either goes to
// a peer NO receive of the record touches (its costs are requested together with the receives': nothing in the level writes
// them), or to the peer of one of the record's receives (the host marks the pair: Op::pad of the send = receive index + 1,
// of the receive = 1), and then the receive's lane hands the rewritten costs over in LDS instead of storing them — the send
// stores the final values.  One round trip per level instead of two, no drain between the rounds.  Same additions in the
// same order as label_ops_body (bit-identical).
template <int A>
__device__ __forceinline__ void label_ops_body_staged(const StagedLevel& st, int64_t first, double* __restrict__ dual, double* __restrict__ lb,
                                                      double (*D)[8][8], double (*S)[8], double (*RS)[8][8]) {
  const int lane = threadIdx.x & 63, q = lane >> 3, j = lane & 7;
  const int64_t idx = first + q;
  const bool live = idx < st.count;
  const UpdRec& rec = st.recs[live ? idx : 0];
  const int n_recv = live ? rec.n_recv : 0, n_send = live ? rec.n_send : 0, on = live ? rec.d0 : 0;
  double* own_g = dual + (live ? rec.dual_off : 0);
  double theta = (live && j < on) ? ld_dual<A>(own_g + j) : 0.0;
  const bool recv = live && j < n_recv, send = live && j < n_send;
  Op o, o2;
  o.peer_dual = 0; o.peer_const = 0; o.omega = 0.0; o.info = 0; o.pd0 = 0; o.pd1 = 0; o.peer = 0; o.len = 0; o.pad = 0; o2 = o;
  if (recv) o = st.ops[idx][j];
  if (send) o2 = st.ops[idx][n_recv + j];
  int tv[SMALL_MAXD], tv2[SMALL_MAXD]; double R[SMALL_MAXD], R2[SMALL_MAXD];
  const int fw = send ? o2.pad : 0;
  double* peer = dual + o.peer_dual; double* peer2 = dual + o2.peer_dual;
#pragma unroll
  for (int r = 0; r < SMALL_MAXD; ++r) {
    const bool in = recv && r < o.pd0, in2 = send && r < o2.pd0;
    tv[r] = in ? st.tab[idx][j][r] : o.pd1;
    tv2[r] = in2 ? st.tab[idx][n_recv + j][r] : o2.pd1;
    R[r] = in ? ld_dual<A>(peer + r) : LPMP_INF;
    R2[r] = (in2 && fw == 0) ? ld_dual<A>(peer2 + r) : LPMP_INF;
  }
  if (g_level_trace && first == 0) { asm volatile("" :: "v"(R[0]), "v"(R2[0]), "v"(theta)); level_stamp(1); }   // costs landed
  if (recv) {
    const int nl = o.pd1;
    st_lb<A>(lb + o.peer, LPMP_NAN);
    double nt = ((o.info >> 6) & 1) ? 0.0 : LPMP_INF;
#pragma unroll
    for (int r = 0; r < SMALL_MAXD; ++r) if (tv[r] >= nl) nt = fmin(nt, R[r]);
    for (int l = 0; l < nl; ++l) {
      double v = LPMP_INF;
#pragma unroll
      for (int r = 0; r < SMALL_MAXD; ++r) if (tv[r] == l) v = fmin(v, R[r]);
      D[q][j][l] = o.omega * (v - nt);
    }
#pragma unroll
    for (int r = 0; r < SMALL_MAXD; ++r) {
      if (r < o.pd0) {
        const double nv = tv[r] < nl ? R[r] + -1.0 * D[q][j][tv[r]] : R[r];
        if (o.pad) RS[q][j][r] = nv;                       // a send of this record takes it from here
        else if (tv[r] < nl) st_dual<A>(peer + r, nv);
      }
    }
  }
  wave_sync();
  if (first == 0) level_stamp(2);                                             // receives done
  for (int k = 0; k < n_recv; ++k) if (j < on) theta += +1.0 * D[q][k][j];   // own(i) += +1.0 * dl(i), receive by receive
  if (live && j < on) S[q][j] = theta;                                        // the state every send starts from
  wave_sync();
  if (send) {
    const int nl = o2.pd1;
    st_lb<A>(lb + o2.peer, LPMP_NAN);
    for (int l = 0; l < o2.len; ++l) D[q][j][l] = o2.omega * S[q][l];
#pragma unroll
    for (int r = 0; r < SMALL_MAXD; ++r) {
      if (r < o2.pd0 && tv2[r] < nl) {
        const double cur = fw > 0 ? RS[q][fw - 1][r] : R2[r];
        st_dual<A>(peer2 + r, cur + +1.0 * D[q][j][tv2[r]]);
      }
    }
  }
  wave_sync();
  for (int k = 0; k < n_send; ++k) if (j < on) theta += -1.0 * D[q][k][j];   // own(i) += -1.0 * dl(i), send by send
  if (live && j == 0) st_lb<A>(lb + rec.factor, LPMP_NAN);
  if (live && j < on) st_dual<A>(own_g + j, theta);
}

template <int G>
__global__ void __launch_bounds__(G == 1 ? 64 * (LL_WAVES + 1) : GenCtx<G>::THREADS)
level_loop_kernel(const ChainLaunch* __restrict__ launches, int n_launches, double* __restrict__ dual, const double* __restrict__ cdata,
                  const int32_t* __restrict__ tabs, double* __restrict__ lb, int flags) {
  using C = GenCtx<G>;
  if constexpr (G == 1) {
    __shared__ double D[LL_WAVES][8][8][8];
    __shared__ double S[LL_WAVES][8][8];
    __shared__ StagedLevel ring[LL_RING];
    __shared__ double RS[LL_WAVES][8][8][8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool plain_rule = !(flags & (SWEEP_RESIDUAL | SWEEP_ADAPTIVE | SWEEP_PRIMAL));
    // The staging pipeline of the wave that runs ahead, one stage per level and iteration (each stage's loads depend on what
    // the previous stage left in LDS an iteration earlier, so an iteration issues all of them at once: one round trip):
    //   iteration l:  records of level l + 3  ->  ops of level l + 2  ->  match tables of level l + 1   (slot = level % LL_RING)
    // and the computing waves read level l from its slot.  stage(a, what) is also run for the first levels before the loop.
    // One iteration of the pipeline for the levels (ar, ao, at) = (l + 3, l + 2, l + 1): ALL loads are issued before anything
    // is written to LDS — three batches of independent loads, one round trip (written stage after stage, each stage's LDS
    // stores waited for its own loads and the three round trips came back in series: no gain over reading the L2 directly).
    // lnr: the ChainLaunch of level ar, loaded an iteration earlier; returns the one of level ar + 1.
    auto stage = [&](int ar, int ao, int at, const ChainLaunch& lnr, bool have_lnr) -> ChainLaunch {
      ChainLaunch next; next.packets = nullptr; next.recs = nullptr; next.ops = nullptr; next.count = 0; next.stride = 0; next.pad = 0;
      if (ar + 1 < n_launches) next = launches[ar + 1];
      // --- issue: records of level ar
      const bool r_ok = have_lnr && ar < n_launches && plain_rule && (lnr.pad & CHAIN_LAUNCH_LABEL_OPS) && lnr.count <= LL_STAGE_RECS;
      double2_t rr[3] = {double2_t{0.0, 0.0}, double2_t{0.0, 0.0}, double2_t{0.0, 0.0}};
      if (r_ok && lane < lnr.count) { const double2_t* src = reinterpret_cast<const double2_t*>(lnr.recs + lane); rr[0] = src[0]; rr[1] = src[1]; rr[2] = src[2]; }
      // --- issue: ops of level ao (its records are in LDS since the last iteration)
      StagedLevel& so = ring[((ao % LL_RING) + LL_RING) % LL_RING];
      const int no = ao < n_launches ? so.count : -1;
      double2_t oo[4][3]; bool o_has[4];           // an Op = three 16-byte pieces (plain vector registers, constant indices)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = lane + 64 * t, r = i / LL_STAGE_OPS, k = i % LL_STAGE_OPS;
        o_has[t] = no >= 0 && r < no && k < so.recs[r].n_recv + so.recs[r].n_send;
        oo[t][0] = oo[t][1] = oo[t][2] = double2_t{0.0, 0.0};
        if (o_has[t]) {
          const double2_t* src = reinterpret_cast<const double2_t*>(so.ops_base + so.recs[r].op_begin + k);
          oo[t][0] = src[0]; oo[t][1] = src[1]; oo[t][2] = src[2];
        }
      }
      // --- issue: match tables (+ the lines of the costs) of level at (its ops are in LDS since the last iteration)
      StagedLevel& st = ring[((at % LL_RING) + LL_RING) % LL_RING];
      const int nt = at < n_launches ? st.count : -1;
      int32_t tv[4][SMALL_MAXD]; bool t_has[4];
      double acc = 0.0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = lane + 64 * t, r = i / LL_STAGE_OPS, k = i % LL_STAGE_OPS;
        t_has[t] = nt >= 0 && r < nt && k < st.recs[r].n_recv + st.recs[r].n_send;
        if (t_has[t]) {
          const Op& o = st.ops[r][k];
          const int32_t* tab = tabs + o.peer_const;
#pragma unroll
          for (int x = 0; x < SMALL_MAXD; ++x) tv[t][x] = x < o.pd0 ? tab[x] : o.pd1;
          const double* pd = dual + o.peer_dual;
          acc += __hip_atomic_load(pd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          acc += __hip_atomic_load(pd + max(peer_dual_size(o) - 1, 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (k == 0) acc += __hip_atomic_load(dual + st.recs[r].dual_off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      // --- everything has landed: into LDS
      if (ar < n_launches) {
        StagedLevel& sr = ring[ar % LL_RING];
        if (lane == 0) { sr.count = r_ok ? (int32_t)lnr.count : -1; sr.pad[0] = lnr.pad; sr.ops_base = lnr.ops; }
        if (r_ok && lane < lnr.count) { double2_t* dst = reinterpret_cast<double2_t*>(&sr.recs[lane]); dst[0] = rr[0]; dst[1] = rr[1]; dst[2] = rr[2]; }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = lane + 64 * t;
        if (o_has[t]) { double2_t* dst = reinterpret_cast<double2_t*>(&so.ops[i / LL_STAGE_OPS][i % LL_STAGE_OPS]); dst[0] = oo[t][0]; dst[1] = oo[t][1]; dst[2] = oo[t][2]; }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = lane + 64 * t;
        if (t_has[t]) {
#pragma unroll
          for (int x = 0; x < SMALL_MAXD; ++x) st.tab[i / LL_STAGE_OPS][i % LL_STAGE_OPS][x] = tv[t][x];
        }
      }
      asm volatile("" :: "v"(acc));
      return next;
    };
    ChainLaunch ln_ahead; ln_ahead.packets = nullptr; ln_ahead.recs = nullptr; ln_ahead.ops = nullptr; ln_ahead.count = 0; ln_ahead.stride = 0; ln_ahead.pad = 0;
    if (threadIdx.x == 0) for (int a = 0; a < LL_RING; ++a) ring[a].count = -1;
    __syncthreads();
    if (wave == LL_WAVES) {                          // fill the pipeline: three iterations ahead of the loop (levels 0, 1, 2 end up staged as far as the loop expects)
      if (n_launches > 0) ln_ahead = launches[0];
      for (int l = -3; l < 0; ++l) { ln_ahead = stage(l + 3, l + 2, l + 1, ln_ahead, true); wave_sync(); }
    }
    __syncthreads();
    for (int l = 0; l < n_launches; ++l) {
      if (g_level_trace && threadIdx.x == 0) g_level_trace[0] = l;
      level_stamp(0);
      if (wave == LL_WAVES) {                        // the wave that runs ahead
        level_stamp_of(6, 64 * LL_WAVES);
        ln_ahead = stage(l + 3, l + 2, l + 1, ln_ahead, true);
        level_stamp_of(7, 64 * LL_WAVES);
        const int la = l + LEVEL_LOOP_AHEAD;         // ... and, further ahead, the touch of everything a level that will NOT be staged reads
        ChainLaunch ln; ln.count = 0; ln.pad = 0;
        if (la < n_launches) ln = launches[la];
        if (la < n_launches && !(plain_rule && (ln.pad & CHAIN_LAUNCH_LABEL_OPS) && ln.count <= LL_STAGE_RECS)) {
          for (int64_t i = lane; i < ln.count; i += 64) {
            const UpdRec r = ln.recs[i];
            double acc = __hip_atomic_load(dual + r.dual_off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const int n_ops = r.n_recv + r.n_send;
            for (int k = 0; k < n_ops; ++k) {
              const Op o = ln.ops[r.op_begin + k];
              const double* pd = dual + o.peer_dual;
              acc += __hip_atomic_load(pd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              acc += __hip_atomic_load(pd + max(peer_dual_size(o) - 1, 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // a peer of this class spans at most two lines
              if ((o.info & 15) == OP_LABELING) acc += (double)tabs[o.peer_const];
            }
            asm volatile("" :: "v"(acc));
          }
        }
      } else {
        const StagedLevel& sl = ring[l % LL_RING];
        ChainLaunch ln;
        if (sl.count >= 0) { ln.packets = nullptr; ln.recs = nullptr; ln.ops = nullptr; ln.count = sl.count; ln.stride = 0; ln.pad = sl.pad[0]; }
        else ln = launches[l];
        if (sl.count >= 0) {                         // records, ops and match tables from LDS
          if (ln.pad & CHAIN_LAUNCH_LABEL_PAIRED) { for (int64_t first = 8 * wave; first < ln.count; first += 8 * LL_WAVES) label_ops_body<ACC_WG, true, true>(ln, first, dual, tabs, lb, D[wave], S[wave], &sl); }
          else { for (int64_t first = 8 * wave; first < ln.count; first += 8 * LL_WAVES) label_ops_body_staged<ACC_WG>(sl, first, dual, lb, D[wave], S[wave], RS[wave]); }
        } else if ((ln.pad & CHAIN_LAUNCH_LABEL_OPS) && plain_rule) {
          if (ln.pad & CHAIN_LAUNCH_LABEL_PAIRED) { for (int64_t first = 8 * wave; first < ln.count; first += 8 * LL_WAVES) label_ops_body<ACC_WG, true>(ln, first, dual, tabs, lb, D[wave], S[wave]); }
          else { for (int64_t first = 8 * wave; first < ln.count; first += 8 * LL_WAVES) label_ops_body<ACC_WG, false>(ln, first, dual, tabs, lb, D[wave], S[wave]); }
        } else if (wave == 0) {
          const int64_t nblk = (ln.count + C::FPB - 1) / C::FPB;
          for (int64_t b = 0; b < nblk; ++b)
            [&] { generic_body<1, ACC_WG>(ln.recs, ln.ops, dual, cdata, tabs, lb, nullptr, nullptr, 0, ln.count, flags, b); }();
        }
      }
      level_stamp(4);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this level's stores are in the L2 before the next level loads
      __syncthreads();
      level_stamp(5);
    }
  } else {
    for (int l = 0; l < n_launches; ++l) {
      const ChainLaunch ln = launches[l];
      const int64_t nblk = (ln.count + C::FPB - 1) / C::FPB;
      for (int64_t b = 0; b < nblk; ++b)
        [&] { generic_body<G, ACC_PLAIN>(ln.recs, ln.ops, dual, cdata, tabs, lb, nullptr, nullptr, 0, ln.count, flags, b); }();
      __syncthreads();
    }
  }
}

// -------------------------------------------------------------------------------------------------
// Potts fast path: L lanes per unary factor; peers are pairwise_potts_factor(L, diff).
// min_b (diff*[a!=b] + m_o[b]) = min(m_o[a], diff + min_{b != a} m_o[b]), with min_{b != a} from the two
// smallest entries of m_o (reference vector::two_min, vector.hxx:348-443).
// Packed like the dense path: the factor's record + ops in one packet, the vectors / coupling of up to 4 receives
// and 4 sends requested before anything is reduced (a 512 x 512 grid is launch-latency bound: what counts is the
// length of one factor's dependent chain).
// -------------------------------------------------------------------------------------------------
template <int L>
__device__ __forceinline__ void two_min_merge(double& a1, double& a2) {   // two smallest over the L-lane group (multiset)
  auto step = [&](double b1, double b2) {
    const double n1 = fmin(a1, b1);
    const double n2 = fmin(fmax(a1, b1), fmin(a2, b2));
    a1 = n1; a2 = n2;
  };
  step(dpp_mov_f64<0xB1>(a1), dpp_mov_f64<0xB1>(a2));
  if constexpr (L >= 4) step(dpp_mov_f64<0x4E>(a1), dpp_mov_f64<0x4E>(a2));
  if constexpr (L >= 8) step(dpp_mov_f64<0x141>(a1), dpp_mov_f64<0x141>(a2));
  if constexpr (L >= 16) step(dpp_mov_f64<0x140>(a1), dpp_mov_f64<0x140>(a2));
  if constexpr (L >= 32) step(shfl_xor_f64(a1, 16), shfl_xor_f64(a2, 16));
}

// VAR: L is the padded width, the label count (<= L) is read at run time; lanes beyond it carry +inf
// A: access policy of the duals; CHAIN: called from the chain executor (see dense_pk_body)
// MBOX: the mailbox form of the chain body (see dense_pk_body and chain_plan.cpp): message vectors between dependent records as
// tagged granules
template <int L, bool VAR, int A, bool CHAIN, bool MBOX = false>
__device__ __forceinline__ void potts_pk_body(const Op* __restrict__ packets, const UpdRec* __restrict__ recs, const Op* __restrict__ ops,
                                              double* __restrict__ dual, const double* __restrict__ cdata, double* __restrict__ lb,
                                              int32_t* __restrict__ primal, int64_t count, int stride, int flags, int64_t block,
                                              const ChainArgs* ca, int ticket, unsigned long long* __restrict__ mbox = nullptr, int n_deps = -1) {
  static_assert(!CHAIN || A == ACC_COH, "chain bodies hand results over through relaxed agent-scope flags: every dual access must be an agent-scope (sc1) access");
  static_assert(!MBOX || (CHAIN && MAILBOX_SENDS <= 4), "the mailbox belongs to the chain executor; this body forwards 4 receives and holds 4 sends");
  constexpr int GPB = 256 / L;
  constexpr int KR = 4, KS = 4;
  constexpr int PIECES = 3 * (1 + pk_indirect_cap(L));
  __shared__ double2_t lds_pk[GPB][PIECES];
  const int grp = threadIdx.x / L, g = threadIdx.x % L;
  const int64_t idx = block * GPB + grp;
  const bool live = idx < count;
  load_packet<L>(lds_pk[grp], packets, recs, ops, idx, stride, live, g);
  const UpdRec* hdr = reinterpret_cast<const UpdRec*>(&lds_pk[grp][0]);
  const Op* lop = reinterpret_cast<const Op*>(&lds_pk[grp][3]);
  const int n_recv = live ? (int)hdr->n_recv : 0;
  const int n_send = live ? (int)hdr->n_send : 0;
  const bool preload_ok = live && (hdr->kind_flags & UPD_PRELOAD_OK) != 0;
  double* own_g = dual + (live ? hdr->dual_off : 0);
  const int Lr = VAR ? (live ? (int)hdr->d0 : 0) : L;
  const bool vl = live && g < Lr;
  bool aborted = false;
  if constexpr (CHAIN) {                        // a Potts neighbour has no table to request ahead: only the coupling
    if (MBOX && n_deps == 0) chain_stamp(*ca, ticket, 1);
    else aborted = !chain_wait(*ca, ticket);
  }
  double theta = vl ? ld_dual<A>(own_g + g) : 0.0;
  double sm[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    sm[k] = 0.0;
    if (preload_ok && k < n_send && vl) {
      const Op& o = lop[n_recv + k];
      sm[k] = ld_dual<A>(dual + o.peer_dual + (((o.info >> 5) & 1) ? Lr : 0) + g);
    }
  }
  double mnew[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) mnew[k] = 0.0;
  int max_recv = n_recv;
#pragma unroll
  for (int m = 32; m >= L; m >>= 1) max_recv = max(max_recv, __shfl_xor(max_recv, m, 64));
  const int lane = threadIdx.x & 63;
  const unsigned long long gmask = (L == 64 ? ~0ull : ((1ull << L) - 1ull)) << (lane - g);

  auto chunk = [&](const int c, auto fw_tag) {
    constexpr bool FW = decltype(fw_tag)::value;
    double msv[KR], mov[KR], diff[KR];
    int64_t msoff[KR];
    int defer[KR];
#pragma unroll
    for (int j = 0; j < KR; ++j) {               // request everything first
      msv[j] = 0.0; mov[j] = VAR ? LPMP_INF : 0.0; diff[j] = 0.0; msoff[j] = 0; defer[j] = 0;
      if (c + j < n_recv) {
        const Op& o = lop[c + j];
        const int side = (o.info >> 5) & 1;
        msoff[j] = o.peer_dual + (side == 0 ? 0 : Lr) + g;
        bool boxed = false;
        if constexpr (MBOX) boxed = (o.info & OP_MAILBOX) != 0;
        if (vl) {
          msv[j] = ld_dual<A>(dual + msoff[j]);
          if (!boxed) mov[j] = ld_dual<A>(dual + o.peer_dual + (side == 0 ? Lr : 0) + g);
        }
        diff[j] = cdata[o.peer_const];
        defer[j] = FW ? o.pad : 0;
      }
    }
    if constexpr (MBOX) {                        // with everything else in flight: the vectors that come by mailbox
#pragma unroll
      for (int j = 0; j < KR; ++j) {
        if (c + j < n_recv) {
          const Op& o = lop[c + j];
          if ((o.info & OP_MAILBOX) && vl) { long long row; __builtin_memcpy(&row, &o.omega, 8); mov[j] = mailbox_take(*ca, mbox + row * (2 * L) + 2 * g, aborted); }
        }
      }
    }
    if constexpr (CHAIN) {                       // every dual awaited before the first store (see dense_pk_body)
      asm volatile("" :: "v"(theta));
#pragma unroll
      for (int k = 0; k < KS; ++k) asm volatile("" :: "v"(sm[k]));
#pragma unroll
      for (int j = 0; j < KR; ++j) { asm volatile("" :: "v"(msv[j])); asm volatile("" :: "v"(mov[j])); asm volatile("" :: "v"(diff[j])); }
    }
#pragma unroll
    for (int j = 0; j < KR; ++j) {
      if (c + j >= max_recv) break;
      const bool act = c + j < n_recv && vl;
      double a1 = mov[j], a2 = LPMP_INF;
      two_min_merge<L>(a1, a2);
      // exactly one lane may take the role of "the" minimum: the lowest lane holding a1
      const unsigned long long holders = __ballot(mov[j] == a1);
      const int first_holder = __ffsll((long long)(holders & gmask)) - 1;
      const double min_except = (lane == first_holder) ? a2 : a1;
      double pb = LPMP_INF;
      if (act) {
        const double q = fmin(0.0 + mov[j], diff[j] + min_except);
        const double delta = msv[j] + q;
        theta += delta;
        const double mn = msv[j] - delta;
        pb = mn + q;
        bool stored = false;
        if constexpr (FW) {
          if (defer[j]) {
#pragma unroll
            for (int q2 = 0; q2 < KR; ++q2) if (q2 == c + j) mnew[q2] = mn;
            stored = true;
          }
        }
        if (!stored) st_dual<A>(dual + msoff[j], mn);
      }
      if (!(FW && defer[j])) {
        pb = vec_min<L, L>(pb);
        if (c + j < n_recv && g == 0) st_lb<A>(lb + lop[c + j].peer, pb);
      }
    }
  };
  if (max_recv > 0) chunk(0, std::true_type{});
  for (int c = KR; c < max_recv; c += KR) chunk(c, std::false_type{});

  if (flags & SWEEP_PRIMAL) {
    const int lab = group_argmin<L, L>(theta, vl, g);
    if (live && g == 0 && (hdr->kind_flags & UPD_PRIMAL)) store_label(primal, hdr->factor, Lr, lab);
  }
  // (see dense_pk_body: the bound of a peer after a send that follows this record's receive through the same vector)
  double snap_min = 0.0;
  if constexpr (!MBOX) snap_min = vec_min<L, L>(vl ? theta : LPMP_INF);
  const bool send_bounds = !MBOX && !(flags & SWEEP_RESIDUAL);
  if (vl && !aborted) {
    const double snap = theta;
    if constexpr (CHAIN) {                          // no load inside the send loop (see dense_pk_body)
      if (!preload_ok) {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
          if (k < n_send) {
            const Op& o = lop[n_recv + k];
            if (o.pad == 0) sm[k] = ld_dual<A>(dual + o.peer_dual + (((o.info >> 5) & 1) ? Lr : 0) + g);
          }
        }
#pragma unroll
        for (int k = 0; k < KS; ++k) asm volatile("" :: "v"(sm[k]));
      }
    }
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      if (k < n_send) {
        const Op& o = lop[n_recv + k];
        double* ms = dual + o.peer_dual + (((o.info >> 5) & 1) ? Lr : 0);
        const int fw = o.pad;
        double cur;
        if (fw > 0) cur = fw == 1 ? mnew[0] : fw == 2 ? mnew[1] : fw == 3 ? mnew[2] : mnew[3];
        else if constexpr (CHAIN) cur = sm[k];
        else cur = preload_ok ? sm[k] : ld_dual<A>(ms + g);
        const double delta = o.omega * snap;
        bool boxed = false;                          // (see dense_pk_body: the reader sets the peer's tracked bound)
        if constexpr (MBOX) {
          boxed = (o.info & OP_MAILBOX) != 0;
          if (boxed && !(flags & SWEEP_RESIDUAL)) mailbox_put(mbox + o.peer_const * (2 * L) + 2 * g, cur + delta, ca->epoch);
        }
        st_dual<A>(ms + g, cur + delta);
        theta -= delta;
        if (g == 0 && !boxed) st_lb<A>(lb + o.peer, fw > 0 && send_bounds ? o.omega * snap_min : LPMP_NAN);
      }
    }
    for (int k = KS; k < n_send; ++k) {
      const Op& o = lop[n_recv + k];
      double* ms = dual + o.peer_dual + (((o.info >> 5) & 1) ? Lr : 0);
      const double delta = o.omega * snap;
      st_dual<A>(ms + g, ld_dual<A>(ms + g) + delta);
      theta -= delta;
      if (g == 0) st_lb<A>(lb + o.peer, LPMP_NAN);
    }
    if (flags & SWEEP_RESIDUAL) {
      double residual = 0.0;
      for (int k = 0; k < n_send; ++k) {
        const Op& o = lop[n_recv + k];
        double* ms = dual + o.peer_dual + (((o.info >> 5) & 1) ? Lr : 0);
        residual += o.omega;
        const double delta = residual * theta;
        const double v = ld_dual<A>(ms + g) + delta;
        if constexpr (MBOX) { if (k < KS && (o.info & OP_MAILBOX)) mailbox_put(mbox + o.peer_const * (2 * L) + 2 * g, v, ca->epoch); }
        st_dual<A>(ms + g, v);
        theta -= delta;
      }
    }
    st_dual<A>(own_g + g, theta);
  }
  { const double ob = vec_min<L, L>(vl ? theta : LPMP_INF); if (live && g == 0) st_lb<A>(lb + hdr->factor, ob); }
}

template <int L, bool VAR, bool NT>
__global__ void __launch_bounds__(256)
sweep_potts_pk_kernel(const Op* __restrict__ packets, const UpdRec* __restrict__ recs, const Op* __restrict__ ops,
                      double* __restrict__ dual, const double* __restrict__ cdata, double* __restrict__ lb,
                      int32_t* __restrict__ primal, int64_t count, int stride, int flags) {
  potts_pk_body<L, VAR, NT ? ACC_NT : ACC_PLAIN, false>(packets, recs, ops, dual, cdata, lb, primal, count, stride, flags, (int64_t)blockIdx.x, nullptr, 0);
}
template <int L, bool VAR, bool MBOX>
__global__ void __launch_bounds__(256)
chain_potts_pk_kernel(ChainArgs ca, const ChainLaunch* __restrict__ launches, double* __restrict__ dual,
                      const double* __restrict__ cdata, double* __restrict__ lb, int32_t* __restrict__ primal, int flags) {
  if constexpr (MBOX) {
    chain_loop_ahead(ca, launches, [&](const ChainLaunch& ln, int64_t block, int ticket, int n_deps) {
      potts_pk_body<L, VAR, ACC_COH, true, true>(ln.packets, ln.recs, ln.ops, dual, cdata, lb, primal, ln.count, ln.stride, flags, block, &ca, ticket, ca.mailbox, n_deps);
    });
  } else {
    chain_loop(ca, launches, [&](const ChainLaunch& ln, int64_t block, int ticket) {
      potts_pk_body<L, VAR, ACC_COH, true>(ln.packets, ln.recs, ln.ops, dual, cdata, lb, primal, ln.count, ln.stride, flags, block, &ca, ticket);
    });
  }
}

// -------------------------------------------------------------------------------------------------
// Streaming path: one wave per unary, pairwise peers of any dims up to BIG_MAX_LABELS, dense or Potts, mixed
// (class KC_DENSE_BIG: more than 32 labels, unaries with both kinds of edges; also what the run-time-dims classes
// fall back to).  Works op by op like the generic kernel, but a
// receive streams the table in blocks of 16 rows x 64 columns (16 coalesced 512-B row segments in flight per
// wave) and reduces without a round trip per row:
//   side 0 (own label = row):    16 per-lane partial minima, one per row, are transposed-and-reduced across the
//                                wave in 4 halving exchanges + 2 all-reduce steps (17 shuffles per 16 rows
//                                instead of 6 per row)
//   side 1 (own label = column): lane-local minimum over the rows, m1[row] broadcast from LDS
// -------------------------------------------------------------------------------------------------
constexpr int BIG_WAVES = 4;
static_assert(BIG_WAVES == BIG_BLOCK_RECORDS, "plan.hpp: records per workgroup of the streaming dense kernel");
// LDS of one wave: theta, m_o, q — `ldim` doubles each, ldim = the launch's largest label count rounded up to 64 (round 6: was
// BIG_MAX_LABELS for every launch, 48 KiB per workgroup, which alone held the kernel at 3 waves per SIMD whatever its registers)
struct BigLds { double* theta; double* mo; double* q; };
// (the one decoding of sweep_bigdim_flags, for the kernels and for the LDS sizes of their launches)
__host__ __device__ __forceinline__ int big_ldim(int flags) { const int k = (flags & SWEEP_BIGDIM_MASK) >> SWEEP_BIGDIM_SHIFT; return k ? 64 * k : BIG_MAX_LABELS; }
// waves (= records) per workgroup and dynamic LDS of a wave-per-unary launch whose waves hold `slabs` slabs of ldim doubles each:
// BIG_WAVES while the workgroup stays within 64 KiB, two above (the streaming class, three slabs, always runs four: 48 KiB at most)
static int big_waves(int flags, int slabs) { return (size_t)BIG_WAVES * slabs * big_ldim(flags) * sizeof(double) <= 65536 ? BIG_WAVES : 2; }
static size_t big_lds_bytes(int flags, int slabs) { return (size_t)big_waves(flags, slabs) * slabs * big_ldim(flags) * sizeof(double); }
static_assert((size_t)BIG_WAVES * 3 * BIG_MAX_LABELS * sizeof(double) <= 65536, "the streaming dense launches assume BIG_WAVES waves per workgroup");
// record and op fields are the same in all lanes of the wave: as scalars, so that row addresses are scalar-base + lane offset
// (one VGPR of offsets for the 16 loads of a block instead of 16 64-bit addresses) and the loop bounds are uniform
__device__ __forceinline__ double uni_f64(double v) { return __longlong_as_double(uni64<64>(__double_as_longlong(v))); }

// v[r] = this lane's partial minimum of row r (16 rows).  Returns the minimum over all 64 lanes of ONE row:
// row 8*bit0 + 4*bit1 + 2*bit2 + bit3 of the lane index.
__device__ __forceinline__ double transpose_min16(double (&v)[16], int lane) {
  {
    const bool up = lane & 1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double keep = up ? v[i + 8] : v[i], send = up ? v[i] : v[i + 8];
      v[i] = fmin(keep, dpp_mov_f64<0xB1>(send));
    }
  }
  {
    const bool up = lane & 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double keep = up ? v[i + 4] : v[i], send = up ? v[i] : v[i + 4];
      v[i] = fmin(keep, dpp_mov_f64<0x4E>(send));
    }
  }
  {
    const bool up = lane & 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const double keep = up ? v[i + 2] : v[i], send = up ? v[i] : v[i + 2];
      v[i] = fmin(keep, shfl_xor_f64(send, 4));
    }
  }
  {
    const bool up = lane & 8;
    const double keep = up ? v[1] : v[0], send = up ? v[0] : v[1];
    v[0] = fmin(keep, shfl_xor_f64(send, 8));
  }
  double r = v[0];
  r = fmin(r, shfl_xor_f64(r, 16));
  r = fmin(r, shfl_xor_f64(r, 32));
  return r;
}

// NT: the tables with non-temporal loads (one launch per step of an HBM-sized model); A: access policy of the duals (ACC_PLAIN in
// the launches of the product.  Round 6 also ran this body inside the chain executor with ACC_COH — joined passes of a 2-colour
// grid with 33 ... 48 labels as one persistent launch in Infinity-Cache order: bit-identical and SLOWER than one launch per step,
// 12.6 against 9.9 ms per pass at 33 labels, 15.4 against 12.1 at 40, 16.8 against 16.6 at 48, and from about 56 labels on the
// window cannot sit in the cache at all — EXPERIMENTS.md K; the kernel went, the policy parameter stayed)
// entry idx of a dense table: a double, or (T32: SWEEP_TAB32) a float that is widened
template <bool NT, bool T32>
__device__ __forceinline__ double ld_tab(const double* __restrict__ T, int64_t idx) {
  if constexpr (T32) return (double)ld_stream<NT>(reinterpret_cast<const float*>(T) + idx);
  else return ld_stream<NT>(T + idx);
}
// ---- The one text of the wave-per-unary kernels (dense_big_body, sweep_diff_kernel; sweep_diff_band_kernel has a copy, see there): everything of a record
// that does not depend on how a receive's q is reduced.  A kernel carves its LDS, calls big_begin, runs each receive as
//   big_recv_begin / stage its constants / wave_sync / fill S.q / wave_sync / big_recv_end
// and ends in big_finish.  What travels with the next op (nothing, {scale, offset}, plus the band word), what is staged into LDS
// and the reduction that fills S.q are the kernel's own.  A: access policy of the duals.  The helpers take the LDS slabs as plain
// pointers and the prefetched values as scalars, not BigLds / BigRecv by reference (EXPERIMENTS.md P: the form that costs a kernel
// at its register cap the least).
__device__ __forceinline__ Op uni_op(Op o) {
  o.peer_dual = uni64<64>(o.peer_dual); o.peer_const = uni64<64>(o.peer_const); o.omega = uni_f64(o.omega);
  o.info = uni<64>(o.info); o.pd0 = uni<64>(o.pd0); o.pd1 = uni<64>(o.pd1); o.peer = uni<64>(o.peer);
  return o;
}
// record i with its fields as scalars; theta = the unary's own duals, into LDS
template <int A>
__device__ __forceinline__ UpdRec big_begin(const UpdRec* recs, int64_t i, double* dual, double* theta, int lane) {
  UpdRec rec = recs[i];
  rec.dual_off = uni64<64>(rec.dual_off); rec.d0 = uni<64>(rec.d0); rec.op_begin = uni<64>(rec.op_begin);
  rec.n_recv = (int16_t)uni<64>((int)rec.n_recv); rec.n_send = (int16_t)uni<64>((int)rec.n_send);
  rec.factor = uni<64>(rec.factor); rec.kind_flags = uni<64>(rec.kind_flags);
  const double* own_g = dual + rec.dual_off;
  for (int i = lane; i < rec.d0; i += 64) theta[i] = ld_dual<A>(own_g + i);
  return rec;
}
// a receive from an R x C factor on `side`: ms = the own side's message vector (Lr entries), Lo = the other side's label count
struct BigRecv { int side, R, C, Lo; double* ms; double ms_pre[2]; };
// requests m_s and stages m_o into LDS.  The own side m_s is requested together with m_o (round 6: it used to be loaded after the
// table had been reduced — one more exposed round trip per receive; one or two values per lane up to 128 labels, later ones are
// loaded where they are needed)
template <int A>
__device__ __forceinline__ BigRecv big_recv_begin(const Op& op, double* dual, double* s_mo, int Lr, int lane) {
  BigRecv r;
  r.side = (op.info >> 5) & 1;
  r.R = op.pd0; r.C = op.pd1;
  r.ms = dual + op.peer_dual + (r.side == 0 ? 0 : r.R);
  const double* mo = dual + op.peer_dual + (r.side == 0 ? r.R : 0);
  r.Lo = r.side == 0 ? r.C : r.R;
#pragma unroll
  for (int j = 0; j < 2; ++j) r.ms_pre[j] = lane + 64 * j < Lr ? ld_dual<A>(r.ms + lane + 64 * j) : 0.0;
  for (int i = lane; i < r.Lo; i += 64) s_mo[i] = ld_dual<A>(mo + i);
  return r;
}
// the update after q is filled: the min-marginal moves from m_s (ms0, ms1 = BigRecv::ms_pre) into theta; the peer's bound after this receive
template <int A>
__device__ __forceinline__ void big_recv_end(double* ms, double ms0, double ms1, int32_t peer, double* theta, const double* q, double* lb, int Lr, int lane) {
  double pb = LPMP_INF;
  for (int i = lane, j = 0; i < Lr; i += 64, ++j) {
    const double msv = j == 0 ? ms0 : j == 1 ? ms1 : ld_dual<A>(ms + i), qv = q[i];
    const double delta = msv + qv;                   // omega = 1: delta = min-marginal
    theta[i] += delta;
    const double mn = msv - delta;
    st_dual<A>(ms + i, mn);
    pb = fmin(pb, mn + qv);
  }
  pb = wave_min(pb);
  if (lane == 0) st_lb<A>(lb + peer, pb);
  wave_sync();
}
// after the receives: the primal label and the sends ...
template <int A>
__device__ __forceinline__ void big_sends(UpdRec rec, const Op* ops, double* dual, double* lb, int32_t* primal,
                                          double* theta, double* q, int flags, int lane) {
  const int Lr = rec.d0;
  if ((flags & SWEEP_PRIMAL) && (rec.kind_flags & UPD_PRIMAL)) {   // first minimiser of theta after the receives
    double bv = LPMP_INF; int bi = 0x7fffffff;
    for (int i = lane; i < Lr; i += 64) { const double x = theta[i]; if (bi == 0x7fffffff || x < bv) { bv = x; bi = i; } }
    const double mn = wave_min(bv);
    int cand = (bi != 0x7fffffff && bv == mn) ? bi : 0x7fffffff;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cand = min(cand, __shfl_xor(cand, m, 64));
    if (lane == 0) store_label(primal, rec.factor, Lr, cand);
  }
  // sends from the state after the receives (kept in q); a lane always owns the same elements: no barrier needed
  for (int i = lane; i < Lr; i += 64) q[i] = theta[i];
  for (int k = 0; k < rec.n_send; ++k) {
    const Op op = uni_op(ops[rec.op_begin + rec.n_recv + k]);
    double* ms = dual + op.peer_dual + (((op.info >> 5) & 1) ? op.pd0 : 0);
    for (int i = lane; i < Lr; i += 64) {
      const double delta = op.omega * q[i];
      st_dual<A>(ms + i, ld_dual<A>(ms + i) + delta);
      theta[i] -= delta;
    }
    if (lane == 0) st_lb<A>(lb + op.peer, LPMP_NAN);
  }
}
// ... and with them the residual rule, the store of theta and the unary's own bound
template <int A>
__device__ __forceinline__ void big_finish(UpdRec rec, const Op* ops, double* dual, double* lb, int32_t* primal,
                                           double* theta, double* q, int flags, int lane) {
  const int Lr = rec.d0;
  big_sends<A>(rec, ops, dual, lb, primal, theta, q, flags, lane);
  if (flags & SWEEP_RESIDUAL) {
    double residual = 0.0;
    for (int k = 0; k < rec.n_send; ++k) {
      const Op op = uni_op(ops[rec.op_begin + rec.n_recv + k]);
      double* ms = dual + op.peer_dual + (((op.info >> 5) & 1) ? op.pd0 : 0);
      residual += op.omega;
      for (int i = lane; i < Lr; i += 64) {
        const double delta = residual * theta[i];
        st_dual<A>(ms + i, ld_dual<A>(ms + i) + delta);
        theta[i] -= delta;
      }
    }
  }
  double* own_g = dual + rec.dual_off;
  double ob = LPMP_INF;
  for (int i = lane; i < Lr; i += 64) { const double x = theta[i]; st_dual<A>(own_g + i, x); ob = fmin(ob, x); }
  ob = wave_min(ob);
  if (lane == 0) st_lb<A>(lb + rec.factor, ob);
}

template <bool NT, int A, bool T32 = false>
__device__ __forceinline__ void dense_big_body(const UpdRec* __restrict__ recs, const Op* __restrict__ ops, double* __restrict__ dual,
                                               const double* __restrict__ cdata, double* __restrict__ lb, int32_t* __restrict__ primal,
                                               int64_t first, int64_t count, int flags, int64_t block) {
  extern __shared__ double big_lds_pool[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t idx = block * BIG_WAVES + wave;
  if (idx >= count) return;
  const int ldim = big_ldim(flags);
  const BigLds S{big_lds_pool + (size_t)wave * 3 * ldim, big_lds_pool + (size_t)wave * 3 * ldim + ldim, big_lds_pool + (size_t)wave * 3 * ldim + 2 * ldim};
  const UpdRec rec = big_begin<A>(recs, first + idx, dual, S.theta, lane);
  const int Lr = rec.d0;
  const int my_row = 8 * (lane & 1) + 4 * ((lane >> 1) & 1) + 2 * ((lane >> 2) & 1) + ((lane >> 3) & 1);
  Op nxt{};
  if (rec.n_recv > 0) nxt = ops[rec.op_begin];
  for (int k = 0; k < rec.n_recv; ++k) {
    const Op op = uni_op(nxt);
    if (k + 1 < rec.n_recv) nxt = ops[rec.op_begin + k + 1];   // requested before this receive's table stream starts
    const double* T = cdata + op.peer_const;
    const BigRecv r = big_recv_begin<A>(op, dual, S.mo, Lr, lane);
    const int side = r.side, R = r.R, C = r.C, Lo = r.Lo;
    wave_sync();
    if (((op.info >> 8) & 15) == LPMP_F_PAIRWISE_POTTS) {
      // q[x] = min(m_o[x], diff + min_{y != x} m_o[y]) from the two smallest entries of m_o (multiset) and the
      // first index that holds the smallest (reference vector::two_min, vector.hxx:348-443)
      const double diff = T[0];
      double a1 = LPMP_INF, a2 = LPMP_INF; int i1 = 0x7fffffff;
      for (int i = lane; i < Lo; i += 64) {
        const double x = S.mo[i];
        if (x < a1 || i1 == 0x7fffffff) { a2 = a1; a1 = x; i1 = i; } else if (x < a2) a2 = x;
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const double b1 = shfl_xor_f64(a1, m), b2 = shfl_xor_f64(a2, m);
        const int j1 = __shfl_xor(i1, m, 64);
        const double n2 = fmin(fmax(a1, b1), fmin(a2, b2));
        if (b1 < a1 || (b1 == a1 && j1 < i1)) i1 = j1;
        a1 = fmin(a1, b1); a2 = n2;
      }
      for (int i = lane; i < Lo; i += 64) S.q[i] = fmin(0.0 + S.mo[i], diff + (i == i1 ? a2 : a1));
    } else if (side == 0) {
      for (int a0 = 0; a0 < R; a0 += 16) {
        double v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = LPMP_INF;
        for (int b0 = 0; b0 < C; b0 += 64) {
          const int b = b0 + lane;
          const bool cb = b < C;
          const double m = cb ? S.mo[b] : 0.0;
          double t[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) t[r] = (cb && a0 + r < R) ? ld_tab<NT, T32>(T, (int64_t)(a0 + r) * C + b) : LPMP_INF;
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = fmin(v[r], t[r] + m);
        }
        const double full = transpose_min16(v, lane);
        if (lane < 16 && a0 + my_row < R) S.q[a0 + my_row] = full;
      }
    } else {
      for (int b0 = 0; b0 < C; b0 += 64) {
        const int b = b0 + lane;
        const bool cb = b < C;
        double v = LPMP_INF;
        for (int a0 = 0; a0 < R; a0 += 16) {
          double t[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) t[r] = (cb && a0 + r < R) ? ld_tab<NT, T32>(T, (int64_t)(a0 + r) * C + b) : LPMP_INF;
#pragma unroll
          for (int r = 0; r < 16; ++r) { const double m = a0 + r < R ? S.mo[a0 + r] : 0.0; v = fmin(v, t[r] + m); }
        }
        if (cb) S.q[b] = v;
      }
    }
    wave_sync();
    big_recv_end<A>(r.ms, r.ms_pre[0], r.ms_pre[1], op.peer, S.theta, S.q, lb, Lr, lane);
  }
  big_finish<A>(rec, ops, dual, lb, primal, S.theta, S.q, flags, lane);
}
// (five waves per SIMD: the body needs 96-101 VGPRs depending on small things, and the kernel is bound by round trips per wave)
template <bool NT>
__global__ void __launch_bounds__(64 * BIG_WAVES, 5)
sweep_dense_big_kernel(const UpdRec* __restrict__ recs, const Op* __restrict__ ops, double* __restrict__ dual,
                       const double* __restrict__ cdata, double* __restrict__ lb, int32_t* __restrict__ primal,
                       int64_t first, int64_t count, int flags) {
  dense_big_body<NT, ACC_PLAIN>(recs, ops, dual, cdata, lb, primal, first, count, flags, (int64_t)blockIdx.x);
}
// float tables (SWEEP_TAB32): one column per lane as above, 4-byte loads
template <bool NT>
__global__ void __launch_bounds__(64 * BIG_WAVES, 5)
sweep_dense_big_f32_kernel(const UpdRec* __restrict__ recs, const Op* __restrict__ ops, double* __restrict__ dual,
                           const double* __restrict__ cdata, double* __restrict__ lb, int32_t* __restrict__ primal,
                           int64_t first, int64_t count, int flags) {
  dense_big_body<NT, ACC_PLAIN, true>(recs, ops, dual, cdata, lb, primal, first, count, flags, (int64_t)blockIdx.x);
}
// -------------------------------------------------------------------------------------------------
// Class KC_DIFF: unaries whose pairwise peers are all DIFF factors (cost(a, b) = scale * D[a - b + d1 - 1], D a vector of
// d0 + d1 - 1 doubles of the shared pool), 2 ... BIG_MAX_LABELS labels.  One wave per unary and op by op: the shared text of
// dense_big_body (big_begin ... big_finish) around another reduction.  A receive writes sD[k] = scale * D[k] into LDS — the ONE multiply of the contract, once per entry —
// and takes q[x] = min_y (sD[x - y + d1 - 1] + m_o[y]) (own side 0; side 1: sD[y - x + d1 - 1]) from there: consecutive lanes read
// consecutive doubles of sD, m_o[y] is a broadcast, a lane keeps up to four own labels 64 apart so that one m_o[y] serves them
// all.  min and + are exact, so the result is the dense body's on the expanded table bit for bit.  No table is read from memory:
// D is 2 ... 8 KB and stays in L2.  (No non-temporal variant: there is no stream it would apply to; SWEEP_NT is ignored.)
// LDS of one wave: theta, m_o, q (ldim doubles each), then sD (2 * ldim), ldim as in the streaming class.
// -------------------------------------------------------------------------------------------------
// q[x] for the own labels x = x0 + lane + 64 i, i < NI.  p0 = the lane's window of sD at y = 0.  Lanes beyond Lr run along
// (uniform loop) and store nothing; their reads stay inside the wave's own LDS: side 0 reaches sD[ldim - 1 + C - 1] at most,
// side 1 reaches back ldim - C doubles before sD at most, into the q / m_o slabs.
template <int NI, bool SIDE1>
__device__ __forceinline__ void diff_minplus(const double* __restrict__ sD, const double* __restrict__ mo, double* __restrict__ q,
                                             int x0, int Lr, int Lo, int C, int lane) {
  const int x = x0 + lane;
  const double* p0 = sD + (SIDE1 ? C - 1 - x : x + C - 1);
  double v[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) v[i] = LPMP_INF;
#pragma unroll 4
  for (int y = 0; y < Lo; ++y) {
    const double m = mo[y];
#pragma unroll
    for (int i = 0; i < NI; ++i) v[i] = fmin(v[i], (SIDE1 ? p0[y - 64 * i] : p0[64 * i - y]) + m);
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) if (x + 64 * i < Lr) q[x + 64 * i] = v[i];
}
template <bool SIDE1>
__device__ __forceinline__ void diff_minplus_all(const double* __restrict__ sD, const double* __restrict__ mo, double* __restrict__ q,
                                                 int Lr, int Lo, int C, int lane) {
  for (int x0 = 0; x0 < Lr; x0 += 256) {
    const int n = (Lr - x0 + 63) >> 6;
    if (n >= 4) diff_minplus<4, SIDE1>(sD, mo, q, x0, Lr, Lo, C, lane);
    else if (n == 3) diff_minplus<3, SIDE1>(sD, mo, q, x0, Lr, Lo, C, lane);
    else if (n == 2) diff_minplus<2, SIDE1>(sD, mo, q, x0, Lr, Lo, C, lane);
    else diff_minplus<1, SIDE1>(sD, mo, q, x0, Lr, Lo, C, lane);
  }
}
// ---- banded form (sweep_diff_band_kernel): D has constant tails, D[k] = D[0] to the bit for k < lo and D[k] = D[n - 1] for k > hi
// (plan.cpp, diff_band; every receive of the launch has a band of at most n / DIFF_BAND_DIV entries).  fl(c + m) is non-decreasing
// in m, so the minimum over the y of a tail is c + (the minimum of m_o over them), bit for bit, and those y are a prefix or a
// suffix of m_o: q[x] = min(window terms, c + pre[...], c + suf[...]) with pre / suf the prefix / suffix minima of m_o.
__device__ __forceinline__ double shfl_up_f64(double v, int d) {
  return __hiloint2double(__shfl_up(__double2hiint(v), d, 64), __shfl_up(__double2loint(v), d, 64));
}
__device__ __forceinline__ double shfl_down_f64(double v, int d) {
  return __hiloint2double(__shfl_down(__double2hiint(v), d, 64), __shfl_down(__double2loint(v), d, 64));
}
__device__ __forceinline__ double shfl_f64(double v, int src) {
  return __hiloint2double(__shfl(__double2hiint(v), src, 64), __shfl(__double2loint(v), src, 64));
}
// pre[i] = min(mo[0 .. i]), suf[i] = min(mo[i .. Lo - 1]): a wave scan per 64 labels, the chunks joined by a carry
__device__ __forceinline__ void diff_band_scans(const double* __restrict__ mo, double* __restrict__ pre, double* __restrict__ suf, int Lo, int lane) {
  double carry = LPMP_INF;
  for (int c0 = 0; c0 < Lo; c0 += 64) {
    const int i = c0 + lane;
    double v = i < Lo ? mo[i] : LPMP_INF;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const double t = shfl_up_f64(v, d); if (lane >= d) v = fmin(v, t); }
    v = fmin(v, carry);
    if (i < Lo) pre[i] = v;
    carry = shfl_f64(v, 63);
  }
  carry = LPMP_INF;
  for (int c0 = ((Lo - 1) >> 6) << 6; c0 >= 0; c0 -= 64) {
    const int i = c0 + lane;
    double v = i < Lo ? mo[i] : LPMP_INF;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const double t = shfl_down_f64(v, d); if (lane + d < 64) v = fmin(v, t); }
    v = fmin(v, carry);
    if (i < Lo) suf[i] = v;
    carry = shfl_f64(v, 0);
  }
}
// q[x] for the own labels x = x0 + lane + 64 i, i < NI.  sB[k - lo] = scale * D[k] for k in [lo, hi], cL / cR = scale * D[0] /
// scale * D[n - 1].  The order of the fmin is fixed: the window entries k = lo ... hi ascending (entry k meets y = x + C - 1 - k on
// side 0, y = k + x - C + 1 on side 1; a y outside [0, Lo) is no term), then the prefix tail, then the suffix tail.  sB[k - lo]
// is a broadcast, consecutive lanes read consecutive doubles of m_o; indices are clamped before they are used, a lane beyond Lr
// runs along and stores nothing.
template <int NI, bool SIDE1>
__device__ __forceinline__ void diff_band_minplus(const double* __restrict__ sB, const double* __restrict__ mo, const double* __restrict__ pre,
                                                  const double* __restrict__ suf, double* __restrict__ q, int x0, int Lr, int Lo, int C,
                                                  int lo, int hi, double cL, double cR, int lane) {
  const int x = x0 + lane;
  double v[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) v[i] = LPMP_INF;
#pragma unroll 2
  for (int k = lo; k <= hi; ++k) {
    const double s = sB[k - lo];
    const int y0 = SIDE1 ? k + x - C + 1 : x + C - 1 - k;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int y = y0 + 64 * i;
      const bool in = (unsigned)y < (unsigned)Lo;
      const double t = s + mo[in ? y : 0];
      v[i] = in ? fmin(v[i], t) : v[i];
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int xi = x + 64 * i;
    const int jp = SIDE1 ? lo + xi - C : xi + C - 2 - hi;       // the tail's y are [0, jp] ...
    const int js = SIDE1 ? hi + xi - C + 2 : xi + C - lo;       // ... and [js, Lo)
    const double tp = (SIDE1 ? cL : cR) + pre[min(max(jp, 0), Lo - 1)];
    const double ts = (SIDE1 ? cR : cL) + suf[min(max(js, 0), Lo - 1)];
    if (jp >= 0) v[i] = fmin(v[i], tp);
    if (js <= Lo - 1) v[i] = fmin(v[i], ts);
    if (xi < Lr) q[xi] = v[i];
  }
}
template <bool SIDE1>
__device__ __forceinline__ void diff_band_minplus_all(const double* __restrict__ sB, const double* __restrict__ mo, const double* __restrict__ pre,
                                                      const double* __restrict__ suf, double* __restrict__ q, int Lr, int Lo, int C,
                                                      int lo, int hi, double cL, double cR, int lane) {
  for (int x0 = 0; x0 < Lr; x0 += 256) {
    const int n = (Lr - x0 + 63) >> 6;
    if (n >= 4) diff_band_minplus<4, SIDE1>(sB, mo, pre, suf, q, x0, Lr, Lo, C, lo, hi, cL, cR, lane);
    else if (n == 3) diff_band_minplus<3, SIDE1>(sB, mo, pre, suf, q, x0, Lr, Lo, C, lo, hi, cL, cR, lane);
    else if (n == 2) diff_band_minplus<2, SIDE1>(sB, mo, pre, suf, q, x0, Lr, Lo, C, lo, hi, cL, cR, lane);
    else diff_band_minplus<1, SIDE1>(sB, mo, pre, suf, q, x0, Lr, Lo, C, lo, hi, cL, cR, lane);
  }
}
constexpr int DIFF_WAVES_PER_SIMD = 6;
// LDS of one wave, in slabs of ldim doubles.  DIFF: theta, m_o, q and sD (2 ldim): four waves while that stays within 64 KiB, two
// above.  ldim is a multiple of 64, so the last size with four waves is 384 labels (60 KiB; 448 would be 70 KiB): launches of more
// than 384 labels run two waves, 40 KiB at 512.  Banded: theta, m_o, q, pre, suf and the band of sD (at most n / DIFF_BAND_DIV <
// ldim / 2 entries): four waves up to 320 labels (60 KiB), two above (48 KiB at 512)
constexpr int DIFF_SLABS = 5, DIFF_BAND_SLABS = 6;
static_assert(DIFF_BAND_DIV >= 2, "the band of sD must fit one slab of ldim doubles: (2 ldim - 1) / DIFF_BAND_DIV <= ldim");
// the band word {lo, hi} the engine keeps in front of every pool entry of its own copy (engine.cpp, lpmp_upload_model)
__device__ __forceinline__ int2 diff_band_word(const double* __restrict__ cdata, int64_t off) { return *reinterpret_cast<const int2*>(cdata + off - 1); }

__global__ void __launch_bounds__(64 * BIG_WAVES, DIFF_WAVES_PER_SIMD)
sweep_diff_kernel(const UpdRec* __restrict__ recs, const Op* __restrict__ ops, double* __restrict__ dual,
                  const double* __restrict__ cdata, double* __restrict__ lb, int32_t* __restrict__ primal,
                  int64_t first, int64_t count, int flags) {
  constexpr int A = ACC_PLAIN;
  extern __shared__ double big_lds_pool[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (idx >= count) return;
  const int ldim = big_ldim(flags);
  double* const slab = big_lds_pool + (size_t)wave * DIFF_SLABS * ldim;
  const BigLds S{slab, slab + ldim, slab + 2 * ldim};
  double* const sD = slab + 3 * ldim;
  const UpdRec rec = big_begin<A>(recs, first + idx, dual, S.theta, lane);
  const int Lr = rec.d0;
  Op nxt{};
  double nscale = 0.0; int64_t noff = 0;               // the next receive's two constant words {scale, offset of D}
  if (rec.n_recv > 0) {
    nxt = ops[rec.op_begin];
    const int64_t pc = uni64<64>(nxt.peer_const);
    nscale = cdata[pc]; noff = shared_table_off(cdata, pc);
  }
  for (int k = 0; k < rec.n_recv; ++k) {
    const Op op = uni_op(nxt);
    const double scale = uni_f64(nscale);
    const double* D = cdata + uni64<64>(noff);
    if (k + 1 < rec.n_recv) nxt = ops[rec.op_begin + k + 1];   // requested before this receive's reduction starts
    const BigRecv r = big_recv_begin<A>(op, dual, S.mo, Lr, lane);   // (m_s is requested together with m_o and D)
    for (int i = lane; i < r.R + r.C - 1; i += 64) sD[i] = scale * D[i];
    wave_sync();
    if (r.side == 0) diff_minplus_all<false>(sD, S.mo, S.q, Lr, r.Lo, r.C, lane);
    else diff_minplus_all<true>(sD, S.mo, S.q, Lr, r.Lo, r.C, lane);
    if (k + 1 < rec.n_recv) {                          // (the next op has arrived long ago: its constants travel during the update below)
      const int64_t pc = uni64<64>(nxt.peer_const);
      nscale = cdata[pc]; noff = shared_table_off(cdata, pc);
    }
    wave_sync();
    big_recv_end<A>(r.ms, r.ms_pre[0], r.ms_pre[1], op.peer, S.theta, S.q, lb, Lr, lane);
  }
  big_finish<A>(rec, ops, dual, lb, primal, S.theta, S.q, flags, lane);
}
// The shifted kernel (launches with a DIFF_SHIFT peer: LevelRange::diff_shift): sweep_diff_kernel with another fill, nothing else —
// the same shared text (big_begin ... big_finish), the same LDS slabs, the same waves, the same reduction, which reads sD only.
// What travels with the next op is {scale, offset of D} and the window {s, n} of the fill, sD[i] = scale * D[clamp(i - (C - 1) + s,
// 0, n - 1)].  A plain DIFF peer of such a launch has no third and fourth word: its window is s = C - 1, n = R + C - 1, by the kind
// in Op::info, and its fill then reads D[i] as the plain kernel does.  The two kernels keep their own lines between the shared
// helpers: with both over one body template the plain kernel compiled to other registers.
struct DiffWin { int s, n; };
__device__ __forceinline__ DiffWin diff_next_win(const Op& nxt, const double* __restrict__ cdata, int64_t pc) {
  if (((uni<64>(nxt.info) >> 8) & 15) == LPMP_F_PAIRWISE_DIFF_SHIFT) return {diff_shift_int(cdata[pc + 2]), diff_shift_n(cdata, pc)};
  const int C = uni<64>(nxt.pd1);
  return {C - 1, uni<64>(nxt.pd0) + C - 1};
}
__global__ void __launch_bounds__(64 * BIG_WAVES, DIFF_WAVES_PER_SIMD)
sweep_diff_shift_kernel(const UpdRec* __restrict__ recs, const Op* __restrict__ ops, double* __restrict__ dual,
                        const double* __restrict__ cdata, double* __restrict__ lb, int32_t* __restrict__ primal,
                        int64_t first, int64_t count, int flags) {
  constexpr int A = ACC_PLAIN;
  extern __shared__ double big_lds_pool[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (idx >= count) return;
  const int ldim = big_ldim(flags);
  double* const slab = big_lds_pool + (size_t)wave * DIFF_SLABS * ldim;
  const BigLds S{slab, slab + ldim, slab + 2 * ldim};
  double* const sD = slab + 3 * ldim;
  const UpdRec rec = big_begin<A>(recs, first + idx, dual, S.theta, lane);
  const int Lr = rec.d0;
  Op nxt{};
  double nscale = 0.0; int64_t noff = 0;               // the next receive's constant words {scale, offset of D} ...
  DiffWin nwin{0, 1};                                  // ... and its window {s, n}
  if (rec.n_recv > 0) {
    nxt = ops[rec.op_begin];
    const int64_t pc = uni64<64>(nxt.peer_const);
    nscale = cdata[pc]; noff = shared_table_off(cdata, pc);
    nwin = diff_next_win(nxt, cdata, pc);
  }
  for (int k = 0; k < rec.n_recv; ++k) {
    const Op op = uni_op(nxt);
    const double scale = uni_f64(nscale);
    const double* D = cdata + uni64<64>(noff);
    const int ws = uni<64>(nwin.s), wn = uni<64>(nwin.n);
    if (k + 1 < rec.n_recv) nxt = ops[rec.op_begin + k + 1];   // requested before this receive's reduction starts
    const BigRecv r = big_recv_begin<A>(op, dual, S.mo, Lr, lane);   // (m_s is requested together with m_o and D)
    // i < R + C - 1 <= 2 ldim - 1: inside the sD slab; the index of D is clamped to [0, n - 1], n from the plan
    for (int i = lane; i < r.R + r.C - 1; i += 64) sD[i] = scale * D[diff_shift_index(i - (r.C - 1), ws, wn)];
    wave_sync();
    if (r.side == 0) diff_minplus_all<false>(sD, S.mo, S.q, Lr, r.Lo, r.C, lane);
    else diff_minplus_all<true>(sD, S.mo, S.q, Lr, r.Lo, r.C, lane);
    if (k + 1 < rec.n_recv) {                          // (the next op has arrived long ago: its constants travel during the update below)
      const int64_t pc = uni64<64>(nxt.peer_const);
      nscale = cdata[pc]; noff = shared_table_off(cdata, pc);
      nwin = diff_next_win(nxt, cdata, pc);
    }
    wave_sync();
    big_recv_end<A>(r.ms, r.ms_pre[0], r.ms_pre[1], op.peer, S.theta, S.q, lb, Lr, lane);
  }
  big_finish<A>(rec, ops, dual, lb, primal, S.theta, S.q, flags, lane);
}
// The banded kernel: sweep_diff_kernel with the reduction of a receive replaced, nothing else.  LDS of one wave: theta, m_o, q, pre,
// suf, the band of sD.  It keeps its own text of the whole body (only uni_op is shared).  The kernel uses all 80 VGPRs of its six
// waves per SIMD: with the shared helpers taking structs by reference, or with big_finish's residual rule or final store in a helper
// in any form, it spills a register (80 VGPRs + 8 B of scratch); sharing big_begin / big_recv_begin / big_recv_end / big_sends and
// keeping only those 16 lines compiled to 80 + 0 and gave the parent's bits, but its pass at 512 x 512 x 128 labels was 0.3 %
// slower than the parent's, outside the parent-against-parent spread in two runs (2.7075 ms against [2.6936, 2.7058]).  A
// wave-uniform slab base avoids the spill (69 VGPRs) but keeps 16 SGPRs in VGPR lanes and changes the waves per SIMD.
// EXPERIMENTS.md P has the forms and the figures; a change to the shared text above is made here too.
__global__ void __launch_bounds__(64 * BIG_WAVES, DIFF_WAVES_PER_SIMD)
sweep_diff_band_kernel(const UpdRec* __restrict__ recs, const Op* __restrict__ ops, double* __restrict__ dual,
                       const double* __restrict__ cdata, double* __restrict__ lb, int32_t* __restrict__ primal,
                       int64_t first, int64_t count, int flags) {
  constexpr int A = ACC_PLAIN;
  extern __shared__ double big_lds_pool[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (idx >= count) return;
  const int ldim = big_ldim(flags);
  double* const slab = big_lds_pool + (size_t)wave * DIFF_BAND_SLABS * ldim;
  BigLds S{slab, slab + ldim, slab + 2 * ldim};
  double* const pre = slab + 3 * ldim; double* const suf = slab + 4 * ldim; double* const sB = slab + 5 * ldim;
  UpdRec rec = recs[first + idx];
  rec.dual_off = uni64<64>(rec.dual_off); rec.d0 = uni<64>(rec.d0); rec.op_begin = uni<64>(rec.op_begin);
  rec.n_recv = (int16_t)uni<64>((int)rec.n_recv); rec.n_send = (int16_t)uni<64>((int)rec.n_send);
  rec.factor = uni<64>(rec.factor); rec.kind_flags = uni<64>(rec.kind_flags);
  const int Lr = rec.d0;
  double* own_g = dual + rec.dual_off;
  for (int i = lane; i < Lr; i += 64) S.theta[i] = ld_dual<A>(own_g + i);
  Op nxt{};
  double nscale = 0.0; int64_t noff = 0;               // the next receive's two constant words {scale, offset of D}
  int2 nband = make_int2(0, -1);                       // ... and the band word of its D
  if (rec.n_recv > 0) {
    nxt = ops[rec.op_begin];
    const int64_t pc = uni64<64>(nxt.peer_const);
    nscale = cdata[pc]; noff = shared_table_off(cdata, pc);
    nband = diff_band_word(cdata, uni64<64>(noff));
  }
  for (int k = 0; k < rec.n_recv; ++k) {
    const Op op = uni_op(nxt);
    const double scale = uni_f64(nscale);
    const double* D = cdata + uni64<64>(noff);
    const int lo = uni<64>(nband.x), hi = uni<64>(nband.y);
    if (k + 1 < rec.n_recv) nxt = ops[rec.op_begin + k + 1];   // requested before this receive's reduction starts
    const int side = (op.info >> 5) & 1;
    const int R = op.pd0, C = op.pd1;
    double* ms = dual + op.peer_dual + (side == 0 ? 0 : R);
    const double* mo = dual + op.peer_dual + (side == 0 ? R : 0);
    const int Lo = side == 0 ? C : R;
    double ms_pre[2];                                  // the own side m_s is requested together with m_o and D
#pragma unroll
    for (int j = 0; j < 2; ++j) ms_pre[j] = lane + 64 * j < Lr ? ld_dual<A>(ms + lane + 64 * j) : 0.0;
    for (int i = lane; i < Lo; i += 64) S.mo[i] = ld_dual<A>(mo + i);
    // the ONE multiply per entry, for the band only; the two tail constants are the products of the end entries
    for (int i = lo + lane; i <= hi; i += 64) sB[i - lo] = scale * D[i];
    const double cL = scale * D[0], cR = scale * D[R + C - 2];
    wave_sync();
    if (k + 1 < rec.n_recv) {                          // the next op has arrived with m_o: its constants travel during the reduction ...
      const int64_t pc = uni64<64>(nxt.peer_const);
      nscale = cdata[pc]; noff = shared_table_off(cdata, pc);
    }
    diff_band_scans(S.mo, pre, suf, Lo, lane);
    wave_sync();
    if (side == 0) diff_band_minplus_all<false>(sB, S.mo, pre, suf, S.q, Lr, Lo, C, lo, hi, cL, cR, lane);
    else diff_band_minplus_all<true>(sB, S.mo, pre, suf, S.q, Lr, Lo, C, lo, hi, cL, cR, lane);
    if (k + 1 < rec.n_recv) nband = diff_band_word(cdata, uni64<64>(noff));   // ... and the band word of its D during the update below
    wave_sync();
    double pb = LPMP_INF;                              // peer's bound after this receive
    for (int i = lane, j = 0; i < Lr; i += 64, ++j) {
      const double msv = j == 0 ? ms_pre[0] : j == 1 ? ms_pre[1] : ld_dual<A>(ms + i), qv = S.q[i];
      const double delta = msv + qv;                   // omega = 1: delta = min-marginal
      S.theta[i] += delta;
      const double mn = msv - delta;
      st_dual<A>(ms + i, mn);
      pb = fmin(pb, mn + qv);
    }
    pb = wave_min(pb);
    if (lane == 0) st_lb<A>(lb + op.peer, pb);
    wave_sync();
  }
  if ((flags & SWEEP_PRIMAL) && (rec.kind_flags & UPD_PRIMAL)) {   // first minimiser of theta after the receives
    double bv = LPMP_INF; int bi = 0x7fffffff;
    for (int i = lane; i < Lr; i += 64) { const double x = S.theta[i]; if (bi == 0x7fffffff || x < bv) { bv = x; bi = i; } }
    const double mn = wave_min(bv);
    int cand = (bi != 0x7fffffff && bv == mn) ? bi : 0x7fffffff;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cand = min(cand, __shfl_xor(cand, m, 64));
    if (lane == 0) store_label(primal, rec.factor, Lr, cand);
  }
  // sends from the state after the receives (kept in q); a lane always owns the same elements: no barrier needed
  for (int i = lane; i < Lr; i += 64) S.q[i] = S.theta[i];
  for (int k = 0; k < rec.n_send; ++k) {
    const Op op = uni_op(ops[rec.op_begin + rec.n_recv + k]);
    double* ms = dual + op.peer_dual + (((op.info >> 5) & 1) ? op.pd0 : 0);
    for (int i = lane; i < Lr; i += 64) {
      const double delta = op.omega * S.q[i];
      st_dual<A>(ms + i, ld_dual<A>(ms + i) + delta);
      S.theta[i] -= delta;
    }
    if (lane == 0) st_lb<A>(lb + op.peer, LPMP_NAN);
  }
  if (flags & SWEEP_RESIDUAL) {
    double residual = 0.0;
    for (int k = 0; k < rec.n_send; ++k) {
      const Op op = uni_op(ops[rec.op_begin + rec.n_recv + k]);
      double* ms = dual + op.peer_dual + (((op.info >> 5) & 1) ? op.pd0 : 0);
      residual += op.omega;
      for (int i = lane; i < Lr; i += 64) {
        const double delta = residual * S.theta[i];
        st_dual<A>(ms + i, ld_dual<A>(ms + i) + delta);
        S.theta[i] -= delta;
      }
    }
  }
  double ob = LPMP_INF;
  for (int i = lane; i < Lr; i += 64) { const double x = S.theta[i]; st_dual<A>(own_g + i, x); ob = fmin(ob, x); }
  ob = wave_min(ob);
  if (lane == 0) st_lb<A>(lb + rec.factor, ob);
}
// The shifted banded kernel (launches with a DIFF_SHIFT peer whose receives all pass the shifted rule: LevelRange::diff_shift_band):
// the text of sweep_diff_band_kernel with the band of a receive computed from the band word of D and the window {s, n} of the
// shifted fill.  The expansion of a receive over i = a - b + C - 1 is D[clamp(i - off, 0, n - 1)], off = C - 1 - s: entries below
// le = clamp(lo + off, 0, R + C - 1) are D[0], entries above he = clamp(hi + off, -1, R + C - 2) are D[n - 1], the ones between
// are D[i - off] — the band moved, clipped to the receive, the clamp continuing both tails — and diff_band_minplus is exact on
// {le, he, scale * D[0], scale * D[n - 1]} as it stands.  A plain DIFF peer has s = C - 1, n = R + C - 1: off = 0.
// Registers: the window's two words beside the band word take the body past the 80 VGPRs of six waves per SIMD, which the banded
// kernel fills to the last one — every six-wave form tried kept 8 to 28 bytes of scratch per lane —, so this kernel
// is built for five (96 VGPRs allowed, 0 scratch).  Up to 128 labels that is one wave per SIMD fewer than the banded kernel; above,
// the LDS of the banded layout sets the occupancy of both.
constexpr int DIFF_SHIFT_BAND_WAVES_PER_SIMD = 5;
__global__ void __launch_bounds__(64 * BIG_WAVES, DIFF_SHIFT_BAND_WAVES_PER_SIMD)
sweep_diff_shift_band_kernel(const UpdRec* __restrict__ recs, const Op* __restrict__ ops, double* __restrict__ dual,
                             const double* __restrict__ cdata, double* __restrict__ lb, int32_t* __restrict__ primal,
                             int64_t first, int64_t count, int flags) {
  constexpr int A = ACC_PLAIN;
  extern __shared__ double big_lds_pool[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (idx >= count) return;
  const int ldim = big_ldim(flags);
  double* const slab = big_lds_pool + (size_t)wave * DIFF_BAND_SLABS * ldim;
  BigLds S{slab, slab + ldim, slab + 2 * ldim};
  double* const pre = slab + 3 * ldim; double* const suf = slab + 4 * ldim; double* const sB = slab + 5 * ldim;
  UpdRec rec = recs[first + idx];
  rec.dual_off = uni64<64>(rec.dual_off); rec.d0 = uni<64>(rec.d0); rec.op_begin = uni<64>(rec.op_begin);
  rec.n_recv = (int16_t)uni<64>((int)rec.n_recv); rec.n_send = (int16_t)uni<64>((int)rec.n_send);
  rec.factor = uni<64>(rec.factor); rec.kind_flags = uni<64>(rec.kind_flags);
  const int Lr = rec.d0;
  double* own_g = dual + rec.dual_off;
  for (int i = lane; i < Lr; i += 64) S.theta[i] = ld_dual<A>(own_g + i);
  Op nxt{};
  double nscale = 0.0; int64_t noff = 0;               // the next receive's two constant words {scale, offset of D}
  int2 nband = make_int2(0, -1);                       // ... the band word of its D ...
  DiffWin nwin{0, 1};                                  // ... and its window {s, n}
  if (rec.n_recv > 0) {
    nxt = ops[rec.op_begin];
    const int64_t pc = uni64<64>(nxt.peer_const);
    nscale = cdata[pc]; noff = shared_table_off(cdata, pc);
    nband = diff_band_word(cdata, uni64<64>(noff));
    nwin = diff_next_win(nxt, cdata, pc);
  }
  for (int k = 0; k < rec.n_recv; ++k) {
    const Op op = uni_op(nxt);
    const double scale = uni_f64(nscale);
    const double* D = cdata + uni64<64>(noff);
    const int ws = uni<64>(nwin.s), wn = uni<64>(nwin.n);
    const int blo = uni<64>(nband.x), bhi = uni<64>(nband.y);
    if (k + 1 < rec.n_recv) nxt = ops[rec.op_begin + k + 1];   // requested before this receive's reduction starts
    const int side = (op.info >> 5) & 1;
    const int R = op.pd0, C = op.pd1;
    double* ms = dual + op.peer_dual + (side == 0 ? 0 : R);
    const double* mo = dual + op.peer_dual + (side == 0 ? R : 0);
    const int Lo = side == 0 ? C : R;
    double ms_pre[2];                                  // the own side m_s is requested together with m_o and D
#pragma unroll
    for (int j = 0; j < 2; ++j) ms_pre[j] = lane + 64 * j < Lr ? ld_dual<A>(ms + lane + 64 * j) : 0.0;
    for (int i = lane; i < Lo; i += 64) S.mo[i] = ld_dual<A>(mo + i);
    // the band of D in the receive's R + C - 1 entries: moved by off = C - 1 - s, clipped to them (wave-uniform).  |off| <= 2^30 +
    // 2^16 fits an int, the band word (below 2^31) plus off need not: those two sums in 64 bits.  hi >= lo - 1, so he >= le - 1:
    // an empty window is le = he + 1, all tails
    const int off = C - 1 - ws;
    const int lo = (int)min(max((long long)blo + off, 0ll), (long long)(R + C - 1));
    const int hi = (int)min(max((long long)bhi + off, -1ll), (long long)(R + C - 2));
    // the ONE multiply per entry, for the window only (k - off is inside the band of D: no clamp; at most (R + C - 1) / DIFF_BAND_DIV
    // entries by the planner's rule: inside the sB slab); the two tail constants are the products of the end entries of D
    for (int i = lo + lane; i <= hi; i += 64) sB[i - lo] = scale * D[i - off];
    const double cL = scale * D[0], cR = scale * D[wn - 1];
    wave_sync();
    if (k + 1 < rec.n_recv) {                          // the next op has arrived with m_o: its constants and window travel during the reduction ...
      const int64_t pc = uni64<64>(nxt.peer_const);
      nscale = cdata[pc]; noff = shared_table_off(cdata, pc);
      nwin = diff_next_win(nxt, cdata, pc);
    }
    diff_band_scans(S.mo, pre, suf, Lo, lane);
    wave_sync();
    if (side == 0) diff_band_minplus_all<false>(sB, S.mo, pre, suf, S.q, Lr, Lo, C, lo, hi, cL, cR, lane);
    else diff_band_minplus_all<true>(sB, S.mo, pre, suf, S.q, Lr, Lo, C, lo, hi, cL, cR, lane);
    if (k + 1 < rec.n_recv) nband = diff_band_word(cdata, uni64<64>(noff));   // ... and the band word of its D during the update below
    wave_sync();
    double pb = LPMP_INF;                              // peer's bound after this receive
    for (int i = lane, j = 0; i < Lr; i += 64, ++j) {
      const double msv = j == 0 ? ms_pre[0] : j == 1 ? ms_pre[1] : ld_dual<A>(ms + i), qv = S.q[i];
      const double delta = msv + qv;                   // omega = 1: delta = min-marginal
      S.theta[i] += delta;
      const double mn = msv - delta;
      st_dual<A>(ms + i, mn);
      pb = fmin(pb, mn + qv);
    }
    pb = wave_min(pb);
    if (lane == 0) st_lb<A>(lb + op.peer, pb);
    wave_sync();
  }
  if ((flags & SWEEP_PRIMAL) && (rec.kind_flags & UPD_PRIMAL)) {   // first minimiser of theta after the receives
    double bv = LPMP_INF; int bi = 0x7fffffff;
    for (int i = lane; i < Lr; i += 64) { const double x = S.theta[i]; if (bi == 0x7fffffff || x < bv) { bv = x; bi = i; } }
    const double mn = wave_min(bv);
    int cand = (bi != 0x7fffffff && bv == mn) ? bi : 0x7fffffff;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cand = min(cand, __shfl_xor(cand, m, 64));
    if (lane == 0) store_label(primal, rec.factor, Lr, cand);
  }
  // sends from the state after the receives (kept in q); a lane always owns the same elements: no barrier needed
  for (int i = lane; i < Lr; i += 64) S.q[i] = S.theta[i];
  for (int k = 0; k < rec.n_send; ++k) {
    const Op op = uni_op(ops[rec.op_begin + rec.n_recv + k]);
    double* ms = dual + op.peer_dual + (((op.info >> 5) & 1) ? op.pd0 : 0);
    for (int i = lane; i < Lr; i += 64) {
      const double delta = op.omega * S.q[i];
      st_dual<A>(ms + i, ld_dual<A>(ms + i) + delta);
      S.theta[i] -= delta;
    }
    if (lane == 0) st_lb<A>(lb + op.peer, LPMP_NAN);
  }
  if (flags & SWEEP_RESIDUAL) {
    double residual = 0.0;
    for (int k = 0; k < rec.n_send; ++k) {
      const Op op = uni_op(ops[rec.op_begin + rec.n_recv + k]);
      double* ms = dual + op.peer_dual + (((op.info >> 5) & 1) ? op.pd0 : 0);
      residual += op.omega;
      for (int i = lane; i < Lr; i += 64) {
        const double delta = residual * S.theta[i];
        st_dual<A>(ms + i, ld_dual<A>(ms + i) + delta);
        S.theta[i] -= delta;
      }
    }
  }
  double ob = LPMP_INF;
  for (int i = lane; i < Lr; i += 64) { const double x = S.theta[i]; st_dual<A>(own_g + i, x); ob = fmin(ob, x); }
  ob = wave_min(ob);
  if (lane == 0) st_lb<A>(lb + rec.factor, ob);
}
// -------------------------------------------------------------------------------------------------
// Updated pairwise factors (dense or Potts), packed form (classes KC_PW_4..32; `right` / `full` schedules, e.g. MPLP-style
// FMCs): the factor is on the right of all its (unary-pairwise) messages.  A receive pulls the whole unary in
// (delta = 1 * theta_u), the sends push omega * min-marginal back.  Same lane layout as sweep_dense_pk_kernel with
// run-time dims (d0 x d1 <= L x L): record + ops in one packet, the factor's OWN table requested right away and
// read ONCE for both sides' min-marginals of the snapshot.
// -------------------------------------------------------------------------------------------------
// T32: the factor's own dense table is stored as floats (SWEEP_TAB32) and widened in the load, nothing else differs
template <int L, bool T32>
__device__ __forceinline__ void pairwise_pk_body(const Op* __restrict__ packets, double* __restrict__ dual, const double* __restrict__ cdata,
                                                 double* __restrict__ lb, int64_t count, int stride) {
  constexpr int G = DenseCfg<L>::G;
  constexpr int CL = L / 2, RPL = 2 * G / L, NL = L / RPL, GPB = 256 / G;
  constexpr int PIECES = 3 * (1 + PW_MAX_OPS);
  __shared__ double2_t lds_pk[GPB][PIECES];
  __shared__ double lds_m1[GPB][L];
  __shared__ double lds_m2[GPB][L];
  __shared__ double lds_q0[GPB][L];
  __shared__ double lds_q1[GPB][L];
  const int grp = threadIdx.x / G, g = threadIdx.x % G;
  const int64_t idx = (int64_t)blockIdx.x * GPB + grp;
  const bool live = idx < count;
  const int c2 = g % CL, rl = g / CL;
  load_packet<G>(lds_pk[grp], packets, nullptr, nullptr, idx, stride, live, g);
  const UpdRec* hdr = reinterpret_cast<const UpdRec*>(&lds_pk[grp][0]);
  const Op* lop = reinterpret_cast<const Op*>(&lds_pk[grp][3]);
  const int n_recv = live ? (int)hdr->n_recv : 0;
  const int n_send = live ? (int)hdr->n_send : 0;
  const int R = live ? hdr->d0 : 0, C = live ? hdr->d1 : 0;
  double* own_g = dual + (live ? hdr->dual_off : 0);
  const double* T = cdata + (live ? hdr->const_off : 0);
  double2_t t[NL];
  if (live && (hdr->kind_flags & 15) == LPMP_F_PAIRWISE_POTTS) {   // diff * [a != b] (reference test/potts_factor.cpp:34-36)
    const double diff = T[0];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int row = i * RPL + rl;
      t[i].x = (row < R && 2 * c2 < C) ? (row == 2 * c2 ? 0.0 : diff) : LPMP_INF;
      t[i].y = (row < R && 2 * c2 + 1 < C) ? (row == 2 * c2 + 1 ? 0.0 : diff) : LPMP_INF;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int row = i * RPL + rl;
      if constexpr (T32) {
        const float* Tr = reinterpret_cast<const float*>(T) + (int64_t)row * C + 2 * c2;   // floats, widened
        t[i].x = (row < R && 2 * c2 < C) ? (double)Tr[0] : LPMP_INF;
        t[i].y = (row < R && 2 * c2 + 1 < C) ? (double)Tr[1] : LPMP_INF;
      } else {
        const double* Tr = T + (int64_t)row * C + 2 * c2;
        t[i].x = (row < R && 2 * c2 < C) ? Tr[0] : LPMP_INF;
        t[i].y = (row < R && 2 * c2 + 1 < C) ? Tr[1] : LPMP_INF;
      }
    }
  }
  double m1 = g < R ? own_g[g] : 0.0;            // message vector of side 0, element g
  double m2 = g < C ? own_g[R + g] : 0.0;        // message vector of side 1, element g
  // receives: delta = 1 * theta_u; the unary gives it up, the factor's vector of that side takes it
#pragma unroll
  for (int k = 0; k < PW_MAX_OPS; ++k) {
    if (k < n_recv) {
      const Op& o = lop[k];
      const int side = (o.info >> 5) & 1;
      if (g < o.len) {
        double* th = dual + o.peer_dual + g;
        const double v = *th;
        const double dl = 1.0 * v;
        *th = v + -1.0 * dl;
        if (side == 0) m1 += +1.0 * dl; else m2 += +1.0 * dl;
      }
      if (g == 0) lb[o.peer] = LPMP_NAN;
    }
  }
  // both min-marginal parts of the state after the receives: q0[a] = min_b T[a][b] + m2[b], q1[b] = min_a T[a][b] + m1[a]
  const double m1s = m1, m2s = m2;
  if (g < L) { lds_m1[grp][g] = m1s; lds_m2[grp][g] = m2s; }
  wave_sync();
  {
    const double2_t mv = *reinterpret_cast<const double2_t*>(&lds_m2[grp][2 * c2]);
    double vx = LPMP_INF, vy = LPMP_INF;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      double v = fmin(t[i].x + mv.x, t[i].y + mv.y);
      v = row_allreduce_min<CL>(v);
      if (c2 == 0) lds_q0[grp][i * RPL + rl] = v;
      const double m1v = lds_m1[grp][i * RPL + rl];
      vx = fmin(vx, t[i].x + m1v);
      vy = fmin(vy, t[i].y + m1v);
    }
#pragma unroll
    for (int m = G / 2; m >= CL; m >>= 1) { vx = fmin(vx, shfl_xor_f64(vx, m)); vy = fmin(vy, shfl_xor_f64(vy, m)); }
    if (rl == 0) { lds_q1[grp][2 * c2] = vx; lds_q1[grp][2 * c2 + 1] = vy; }
  }
  wave_sync();
  const double q0 = g < L ? lds_q0[grp][g] : 0.0, q1 = g < L ? lds_q1[grp][g] : 0.0;
  // sends: delta = omega * min-marginal of the snapshot
#pragma unroll
  for (int k = 0; k < PW_MAX_OPS; ++k) {
    if (k < n_send) {
      const Op& o = lop[n_recv + k];
      const int side = (o.info >> 5) & 1;
      if (g < o.len) {
        const double dl = o.omega * (side == 0 ? m1s + q0 : m2s + q1);
        double* th = dual + o.peer_dual + g;
        *th += +1.0 * dl;
        if (side == 0) m1 += -1.0 * dl; else m2 += -1.0 * dl;
      }
      if (g == 0) lb[o.peer] = LPMP_NAN;
    }
  }
  if (g < R) own_g[g] = m1;
  if (g < C) own_g[R + g] = m2;
  if (live && g == 0) lb[hdr->factor] = LPMP_NAN;
}
template <int L>
__global__ void __launch_bounds__(256)
sweep_pairwise_pk_kernel(const Op* __restrict__ packets, double* __restrict__ dual, const double* __restrict__ cdata,
                         double* __restrict__ lb, int64_t count, int stride) {
  pairwise_pk_body<L, false>(packets, dual, cdata, lb, count, stride);
}
template <int L>
__global__ void __launch_bounds__(256)
sweep_pairwise_pk_f32_kernel(const Op* __restrict__ packets, double* __restrict__ dual, const double* __restrict__ cdata,
                             double* __restrict__ lb, int64_t count, int stride) {
  pairwise_pk_body<L, true>(packets, dual, cdata, lb, count, stride);
}

// -------------------------------------------------------------------------------------------------
// Lower bound (reference LP::LowerBound, LP_MP.h:1507-1518): per-factor bound, then a fixed-order sum.
// -------------------------------------------------------------------------------------------------
// the bound of factor record r, by one wave (any kind); the same value in every lane.  The kind is decided outside the loops; the
// cost expressions are pw_cost's, one multiply for SHARED / DIFF / DIFF_SHIFT.
__device__ __forceinline__ double factor_lb(const LbRec& r, const double* __restrict__ dual, const double* __restrict__ cdata, int tab32, int lane) {
  const int kind = r.kind_flags & 15, flags = r.kind_flags >> 4;
  const double* d = dual + r.dual_off;
  if (kind == LPMP_F_VECTOR) {
    double v = LPMP_INF;
    for (int i = lane; i < r.d0; i += 64) v = fmin(v, d[i]);
    double lb = wave_min(v);
    if ((flags & LPMP_FF_IMPLICIT_ORIGIN) && 0.0 < lb) lb = 0.0;
    return lb;
  }
  // min_a ( m1[a] + min_b (T[a][b] + m2[b]) ): lanes sweep the table row-major (coalesced)
  const int d0 = r.d0, d1 = r.d1;
  double best = LPMP_INF;
  if (kind == LPMP_F_PAIRWISE_DENSE) {
    const double* T = cdata + r.const_off;
    const float* T32 = reinterpret_cast<const float*>(T);
    for (int a = 0; a < d0; ++a) {
      double v = LPMP_INF;
      for (int b = lane; b < d1; b += 64) v = fmin(v, (tab32 ? (double)T32[(int64_t)a * d1 + b] : T[(int64_t)a * d1 + b]) + d[d0 + b]);
      v = wave_min(v);
      best = fmin(best, d[a] + v);
    }
  } else if (kind == LPMP_F_PAIRWISE_SHARED) {
    const double scale = cdata[r.const_off];
    const double* V = cdata + shared_table_off(cdata, r.const_off);
    for (int a = 0; a < d0; ++a) {
      double v = LPMP_INF;
      for (int b = lane; b < d1; b += 64) v = fmin(v, scale * V[(int64_t)a * d1 + b] + d[d0 + b]);
      v = wave_min(v);
      best = fmin(best, d[a] + v);
    }
  } else if (kind == LPMP_F_PAIRWISE_DIFF) {
    const double scale = cdata[r.const_off];
    const double* D = cdata + shared_table_off(cdata, r.const_off) + (d1 - 1);
    for (int a = 0; a < d0; ++a) {
      double v = LPMP_INF;
      for (int b = lane; b < d1; b += 64) v = fmin(v, scale * D[a - b] + d[d0 + b]);
      v = wave_min(v);
      best = fmin(best, d[a] + v);
    }
  } else if (kind == LPMP_F_PAIRWISE_DIFF_SHIFT) {
    const double scale = cdata[r.const_off];
    const double* D = cdata + shared_table_off(cdata, r.const_off);
    const int s = diff_shift_int(cdata[r.const_off + 2]), n = diff_shift_n(cdata, r.const_off);
    for (int a = 0; a < d0; ++a) {
      double v = LPMP_INF;
      for (int b = lane; b < d1; b += 64) v = fmin(v, scale * D[diff_shift_index(a - b, s, n)] + d[d0 + b]);
      v = wave_min(v);
      best = fmin(best, d[a] + v);
    }
  } else {
    const double diff = cdata[r.const_off];
    for (int a = 0; a < d0; ++a) {
      double v = LPMP_INF;
      for (int b = lane; b < d1; b += 64) v = fmin(v, (a == b ? 0.0 : diff) + d[d0 + b]);
      v = wave_min(v);
      best = fmin(best, d[a] + v);
    }
  }
  return best;
}
// one wave per factor, every factor
__global__ void __launch_bounds__(256)
factor_lb_kernel(const LbRec* __restrict__ recs, const double* __restrict__ dual, const double* __restrict__ cdata,
                 double* __restrict__ out, int64_t count, int tab32) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * 4 + wave;
  if (f >= count) return;
  const double lb = factor_lb(recs[f], dual, cdata, tab32, lane);
  if (lane == 0) out[f] = lb;
}

// the same for an explicit list of factors (the ones whose tracked bound is stale)
__global__ void __launch_bounds__(256)
factor_lb_list_kernel(const LbRec* __restrict__ recs, const double* __restrict__ dual, const double* __restrict__ cdata,
                      double* __restrict__ out, const int32_t* __restrict__ list, int64_t count, int tab32) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  if (i >= count) return;
  const int32_t f = list[i];
  const double lb = factor_lb(recs[f], dual, cdata, tab32, lane);
  if (lane == 0) out[f] = lb;
}

// indices of the factors whose tracked bound is NaN
__global__ void __launch_bounds__(256)
lb_collect_stale_kernel(const double* __restrict__ lb, int64_t n, int32_t* __restrict__ list, unsigned long long* __restrict__ counter) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    if (lb[i] != lb[i]) list[atomicAdd(counter, 1ull)] = (int32_t)i;
}

// dense L x L pairwise bound with the table layout of the dense fast path (G lanes per factor, DenseCfg)
template <int L>
__global__ void __launch_bounds__(256)
dense_lb_kernel(const LbRec* __restrict__ recs, const double* __restrict__ dual, const double* __restrict__ cdata,
                double* __restrict__ out, int64_t first, int64_t count, int tab32) {
  constexpr int G = DenseCfg<L>::G;
  constexpr int CL = L / 2, RPL = 2 * G / L, NL = L / RPL, GPB = 256 / G;
  __shared__ double lds_m[GPB][2 * L];
  const int grp = threadIdx.x / G, g = threadIdx.x % G;
  const int64_t idx = (int64_t)blockIdx.x * GPB + grp;
  const bool live = idx < count;
  const int c2 = g % CL, rl = g / CL;
  LbRec r;
  if (live) r = recs[first + idx]; else { r.dual_off = 0; r.const_off = 0; }
  const double* T = cdata + r.const_off;
  const double* d = dual + r.dual_off;
  double2_t t[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    if (!live) t[i] = double2_t{0.0, 0.0};
    else if (tab32) { const float2_t f = *reinterpret_cast<const float2_t*>(reinterpret_cast<const float*>(T) + (int64_t)i * 2 * G + 2 * g); t[i] = double2_t{(double)f.x, (double)f.y}; }
    else t[i] = *reinterpret_cast<const double2_t*>(T + (int64_t)i * 2 * G + 2 * g);
  }
  for (int i = g; i < 2 * L; i += G) lds_m[grp][i] = live ? d[i] : 0.0;
  wave_sync();
  const double2_t m2 = *reinterpret_cast<const double2_t*>(&lds_m[grp][L + 2 * c2]);
  double best = LPMP_INF;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    double v = fmin(t[i].x + m2.x, t[i].y + m2.y);
    v = row_allreduce_min<CL>(v);
    best = fmin(best, lds_m[grp][i * RPL + rl] + v);
  }
#pragma unroll
  for (int m = G / 2; m >= CL; m >>= 1) best = fmin(best, shfl_xor_f64(best, m));
  if (live && g == 0) out[first + idx] = best;
}

// ---- primal rounding: bookkeeping around the sweep (engine.cpp) ------------------------------------
// conditionally_init_primal of every factor a primal pass touches (reference factors_messages.hxx:3302-3309; all of
// them carry the same time stamp, so the host decides whether this runs)
__global__ void __launch_bounds__(256)
primal_init_kernel(const PrimalInit* __restrict__ list, int64_t n, int32_t* __restrict__ primal) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const PrimalInit r = list[i];
  primal[2 * (int64_t)r.f] = r.a;
  primal[2 * (int64_t)r.f + 1] = r.b;
}
// propagate_primal_through_messages of the rounded unaries: right.primal_[side] = left.primal when that is set
// (MessageContainer::ComputeRightFromLeftPrimal, reference factors_messages.hxx:1313-1328)
__global__ void __launch_bounds__(256)
primal_propagate_kernel(const PrimalLink* __restrict__ links, int64_t n, int32_t* __restrict__ primal) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const PrimalLink l = links[i];
  const int32_t x = primal[2 * (int64_t)l.u];
  if (x < l.dim) primal[2 * (int64_t)l.p + l.side] = x;
}
// ---- conditional rounding from the duals (lpmp_decode_primal) -------------------------------------------------
// One level of a decode sweep.  A unary u takes the first minimiser of
//   c[x] = theta_u[x] + sum over its counted links, in link order, of (cost_p(x, x_v) + m_s[x])      (the inner sum first)
// where x_v is the label the unary on the other side of pairwise factor p holds and m_s p's message vector of u's side.  Counted:
// every link (DECODE_ALL, a refinement sweep) or the links whose other unary has a lower level than this launch (the initial
// sweep: exactly the neighbours that are earlier in the order, plan.hpp).  Nothing but u's label is written, so the unaries of a
// level — never neighbours — are independent.  G lanes per unary stride over x; a lane holds CH entries of c in registers, and
// a unary of more than G * CH labels is done chunk by chunk (the links are read again; the running minimum keeps the first).
// Per link: the other label is one load per group, m_s a coalesced vector load, the table line the contiguous row for side 1 and
// the column (stride pd1) for side 0; the next link's record, label and m_s are requested before the current line is added.
template <int G>
__device__ __forceinline__ double decode_min(double v) {
#pragma unroll
  for (int m = G / 2; m >= 1; m >>= 1) v = fmin(v, shfl_xor_f64(v, m));
  return v;
}
template <int G>
__device__ __forceinline__ int decode_min(int v) {
#pragma unroll
  for (int m = G / 2; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}
template <int G, int CH>
struct DecodeFetch {      // what is requested one link ahead
  DecodeLink lk; int xv; double ms[CH]; bool use;
  __device__ __forceinline__ void load(const DecodeLink* __restrict__ links, int k, int n, const double* __restrict__ dual,
                                       const int32_t* __restrict__ primal, int level, int flags, int base, int g, int d0) {
    use = false;
    if (k >= n) return;
    lk = links[k];
    use = (flags & DECODE_ALL) || lk.level < level;
    if (!use) return;
    const int od = lk.side == 0 ? lk.pd1 : lk.pd0;                 // labels of the other unary
    xv = min(max(primal[2 * (int64_t)lk.other], 0), od - 1);        // (a counted neighbour always holds a label: the clamp only keeps a stray array in bounds)
    const double* m = dual + lk.peer_dual + (lk.side ? lk.pd0 : 0);
#pragma unroll
    for (int j = 0; j < CH; ++j) { const int x = base + j * G + g; ms[j] = x < d0 ? m[x] : 0.0; }
  }
};
template <int G, int CH>
__global__ void __launch_bounds__(256)
decode_kernel(const DecodeRec* __restrict__ recs, const DecodeLink* __restrict__ links, const double* __restrict__ dual,
              const double* __restrict__ cdata, int32_t* __restrict__ primal, int64_t first, int64_t count, int level, int flags, int tab32) {
  constexpr int GPB = 256 / G, NONE = 0x7fffffff;
  const int grp = threadIdx.x / G, g = threadIdx.x % G;
  const int64_t idx = (int64_t)blockIdx.x * GPB + grp;
  const bool live = idx < count;
  DecodeRec r;
  if (live) r = recs[first + idx]; else { r.dual_off = 0; r.d0 = 0; r.link_begin = 0; r.n_links = 0; r.factor = 0; }
  const int d0 = r.d0, n = r.n_links;
  const DecodeLink* lks = links + r.link_begin;
  const double* th = dual + r.dual_off;
  double best = LPMP_INF; int label = NONE;
  for (int base = 0; base < d0; base += G * CH) {
    double c[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) { const int x = base + j * G + g; c[j] = x < d0 ? th[x] : LPMP_INF; }
    DecodeFetch<G, CH> cur, nxt;
    cur.load(lks, 0, n, dual, primal, level, flags, base, g, d0);
    for (int k = 0; k < n; ++k) {
      nxt.load(lks, k + 1, n, dual, primal, level, flags, base, g, d0);
      if (cur.use) {
        const DecodeLink& lk = cur.lk;
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int x = base + j * G + g;
          if (x < d0) {
            const double t = lk.side == 0 ? pw_cost(cdata, lk.peer_const, lk.kind, lk.pd1, x, cur.xv, tab32)
                                          : pw_cost(cdata, lk.peer_const, lk.kind, lk.pd1, cur.xv, x, tab32);
            c[j] = c[j] + (t + cur.ms[j]);
          }
        }
      }
      cur = nxt;
    }
    // first minimiser of the chunk: per lane in ascending x, then value / index butterflies over the group
    double bv = LPMP_INF; int bi = NONE;
#pragma unroll
    for (int j = 0; j < CH; ++j) { const int x = base + j * G + g; if (x < d0 && (bi == NONE || c[j] < bv)) { bv = c[j]; bi = x; } }
    const double mn = decode_min<G>(bv);
    const int cand = decode_min<G>((bi != NONE && bv == mn) ? bi : NONE);
    if (label == NONE || mn < best) { best = mn; label = cand; }
  }
  if (live && g == 0 && label != NONE) primal[2 * (int64_t)r.factor] = label;
}

// ---- path moves: exact relabelling of whole paths (lpmp_path_moves) ----------------------------------------------
// One launch is the paths of one group that share a form; they are independent by construction (no pairwise factor joins two of
// them), so no workgroup waits for another.  T threads per path — a wave (four paths per workgroup) while no node has more than
// PATH_WAVE_MAX labels, the workgroup above — with thread y holding label y (and y + T).  Per node i, in path order:
//   n_i[y] = theta[y] + its links in ascending message index: m_s[y] for a path edge, (cost line at the other unary's label + m_s[y])
//            otherwise (the decode's sum)
//   f_i[y] = min_x (f_{i-1}[x] + c_i(x, y)) + n_i[y], strict < in ascending x (the first minimiser is the back-pointer)
// f lives in LDS, double buffered (one barrier per node); c_i goes through pw_cost entry by entry, the exact O(L^2) form for every
// kind.  n_{i+1} does not depend on f: its record, labels, lines and vectors are requested before the min-plus of node i.  The
// back-pointers go to the scratch buffer (a byte each while the previous node has at most 256 labels, two above) and thread 0
// walks them backwards at the end; nothing but the labels of the path's nodes is written to primal.
template <int T>
__device__ __forceinline__ void path_sync() { if (T == 64) wave_sync(); else __syncthreads(); }
__device__ __forceinline__ double path_node_cost(const PathNode& nd, const PathLink* __restrict__ links, const double* __restrict__ dual,
                                                 const double* __restrict__ cdata, const int32_t* primal, int y, int tab32) {
  double n = dual[nd.dual_off + y];
  const PathLink* lks = links + nd.link_begin;
  for (int k = 0; k < nd.n_links; ++k) {
    const PathLink lk = lks[k];
    const double ms = dual[lk.vec_off + y];
    if (lk.on_path) { n = n + ms; continue; }
    const int xv = min(max(primal[2 * (int64_t)lk.other], 0), lk.od - 1);   // (an unset or stray label: the clamp keeps the read inside the table)
    const double t = lk.side == 0 ? pw_cost(cdata, lk.peer_const, lk.kind, lk.pd1, y, xv, tab32) : pw_cost(cdata, lk.peer_const, lk.kind, lk.pd1, xv, y, tab32);
    n = n + (t + ms);
  }
  return n;
}
// g = min_x (fp[x] + c(x, y)) and b = the smallest minimising x (g = +inf, b = 0 on entry), c(x, y) = cost(x, y) with the previous
// node on side 0 of the edge and cost(y, x) otherwise.  Ascending x, strict <; the costs of PATH_CHUNK consecutive x are requested
// before the first of them is added (an x beyond dp - 1 requests entry dp - 1 again and is not counted)
constexpr int PATH_CHUNK = 16;
template <int KIND, int T32>
__device__ __forceinline__ void path_min_plus(const double* __restrict__ cdata, int64_t coff, int d1, int prev_side, const double* fp, int dp, int y,
                                              double& g, int& b) {
  for (int x0 = 0; x0 < dp; x0 += PATH_CHUNK) {
    double c[PATH_CHUNK];
    if (prev_side == 0) {
#pragma unroll
      for (int j = 0; j < PATH_CHUNK; ++j) c[j] = pw_cost(cdata, coff, KIND, d1, min(x0 + j, dp - 1), y, T32);
    } else {
#pragma unroll
      for (int j = 0; j < PATH_CHUNK; ++j) c[j] = pw_cost(cdata, coff, KIND, d1, y, min(x0 + j, dp - 1), T32);
    }
#pragma unroll
    for (int j = 0; j < PATH_CHUNK; ++j) {
      const int x = x0 + j;
      const double v = fp[min(x, dp - 1)] + c[j];
      if (x < dp && v < g) { g = v; b = x; }
    }
  }
}
template <int T>
__global__ void __launch_bounds__(256)
path_moves_kernel(const PathRec* __restrict__ paths, const PathNode* __restrict__ nodes, const PathLink* __restrict__ links,
                  const double* __restrict__ dual, const double* __restrict__ cdata, int32_t* primal, unsigned char* back,
                  int64_t first, int64_t count, int tab32) {
  constexpr int PPB = 256 / T, W = T == 64 ? PATH_WAVE_MAX : PATH_MAX_LABELS, NY = W / T, NONE = 0x7fffffff;
  __shared__ double f[PPB][2][W];
  __shared__ double red_v[4];
  __shared__ int red_i[4];
  const int team = threadIdx.x / T, t = threadIdx.x % T;
  const int64_t idx = (int64_t)blockIdx.x * PPB + team;
  if (idx >= count) return;          // (T == 64: a whole wave, and the wave form has no workgroup barrier; T == 256: never)
  const PathRec pr = paths[first + idx];
  const PathNode* nds = nodes + pr.node_begin;
  const int k = pr.n_nodes;
  PathNode nd = nds[0], nx = nd;
  double nc[NY], nn[NY];
#pragma unroll
  for (int j = 0; j < NY; ++j) { const int y = t + j * T; nc[j] = y < nd.d0 ? path_node_cost(nd, links, dual, cdata, primal, y, tab32) : 0.0; nn[j] = 0.0; }
  int dp = 0;
  for (int i = 0; i < k; ++i) {
    double* fc = f[team][i & 1];
    const double* fp = f[team][(i & 1) ^ 1];
    const bool more = i + 1 < k;
    if (more) {
      nx = nds[i + 1];
#pragma unroll
      for (int j = 0; j < NY; ++j) { const int y = t + j * T; nn[j] = y < nx.d0 ? path_node_cost(nx, links, dual, cdata, primal, y, tab32) : 0.0; }
    }
#pragma unroll
    for (int j = 0; j < NY; ++j) {
      const int y = t + j * T;
      if (y >= nd.d0) continue;
      if (i == 0) { fc[y] = nc[j]; continue; }
      double g = LPMP_INF; int b = 0;
      switch (nd.edge_kind) {      // (wave-uniform: pw_cost with the kind known, so that the loads of a chunk are issued together)
        case LPMP_F_PAIRWISE_DENSE:
          if (tab32) path_min_plus<LPMP_F_PAIRWISE_DENSE, 1>(cdata, nd.edge_const, nd.edge_d1, nd.edge_prev_side, fp, dp, y, g, b);
          else path_min_plus<LPMP_F_PAIRWISE_DENSE, 0>(cdata, nd.edge_const, nd.edge_d1, nd.edge_prev_side, fp, dp, y, g, b);
          break;
        case LPMP_F_PAIRWISE_SHARED: path_min_plus<LPMP_F_PAIRWISE_SHARED, 0>(cdata, nd.edge_const, nd.edge_d1, nd.edge_prev_side, fp, dp, y, g, b); break;
        case LPMP_F_PAIRWISE_DIFF: path_min_plus<LPMP_F_PAIRWISE_DIFF, 0>(cdata, nd.edge_const, nd.edge_d1, nd.edge_prev_side, fp, dp, y, g, b); break;
        case LPMP_F_PAIRWISE_DIFF_SHIFT: path_min_plus<LPMP_F_PAIRWISE_DIFF_SHIFT, 0>(cdata, nd.edge_const, nd.edge_d1, nd.edge_prev_side, fp, dp, y, g, b); break;
        default: path_min_plus<LPMP_F_PAIRWISE_POTTS, 0>(cdata, nd.edge_const, nd.edge_d1, nd.edge_prev_side, fp, dp, y, g, b); break;
      }
      if (nd.back_wide) reinterpret_cast<unsigned short*>(back + nd.back_off)[y] = (unsigned short)b;
      else back[nd.back_off + y] = (unsigned char)b;
      fc[y] = g + nc[j];
    }
    path_sync<T>();
    dp = nd.d0;
    if (more) {
      nd = nx;
#pragma unroll
      for (int j = 0; j < NY; ++j) nc[j] = nn[j];
    }
  }
  // the first minimiser of the last f: per thread in ascending y, then value / index butterflies over the wave (and the waves)
  const double* fl = f[team][(k - 1) & 1];
  double bv = LPMP_INF; int bi = NONE;
#pragma unroll
  for (int j = 0; j < NY; ++j) { const int y = t + j * T; if (y < nd.d0 && (bi == NONE || fl[y] < bv)) { bv = fl[y]; bi = y; } }
  double mn = decode_min<64>(bv);
  int label = decode_min<64>((bi != NONE && bv == mn) ? bi : NONE);
  if (T > 64) {
    if ((threadIdx.x & 63) == 0) { red_v[threadIdx.x >> 6] = mn; red_i[threadIdx.x >> 6] = label; }
    __syncthreads();
    mn = LPMP_INF; label = NONE;
    for (int w = 0; w < T / 64; ++w)
      if (red_i[w] != NONE && (label == NONE || red_v[w] < mn || (red_v[w] == mn && red_i[w] < label))) { mn = red_v[w]; label = red_i[w]; }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the back-pointers the other threads stored
  if (t != 0) return;
  int x = label;
  for (int i = k - 1; i >= 1; --i) {
    const PathNode b = nds[i];
    primal[2 * (int64_t)b.factor] = x;
    x = b.back_wide ? (int)reinterpret_cast<const unsigned short*>(back + b.back_off)[x] : (int)back[b.back_off + x];
  }
  primal[2 * (int64_t)nds[0].factor] = x;
}

// ---- forest moves: exact relabelling of induced forests (lpmp_forest_moves) ---------------------------------------
// One launch of the up kernel is the nodes of one group, one height and one form; their children are lower and were done by
// earlier launches on the stream, so no workgroup waits for another.  T threads per node (a wave — four nodes per workgroup —
// while neither the node nor its parent has more than PATH_WAVE_MAX labels, the workgroup above):
//   thread x:  f[x] = n[x] (path_node_cost: the tree edges count with their message vector only), then + the row g_c[x] of every
//              child in child order; f goes to LDS, one barrier
//   a non-root node, thread y over the PARENT's labels:  g[y] = min_x (f[x] + c(x, y)), strict < in ascending x (path_min_plus),
//              stored with the back-pointer to the scratch
//   a root:    the first minimiser of f (the value / index reduction of path_moves_kernel) is its label
// The down kernel takes one depth level >= 1 per launch, a thread per node: its label is its back-pointer at the parent's label.
// Off-tree neighbours are never members of the group (the planner refuses such a set), so the labels read by the node costs are
// those the group started on whatever the launches have written.
template <int T>
__global__ void __launch_bounds__(256)
forest_up_kernel(const int32_t* __restrict__ list, const ForestNode* __restrict__ nodes, const int64_t* __restrict__ child_g,
                 const PathLink* __restrict__ links, const double* __restrict__ dual, const double* __restrict__ cdata, int32_t* primal,
                 double* rows, unsigned char* back, int64_t first, int64_t count, int tab32) {
  constexpr int PPB = 256 / T, W = T == 64 ? PATH_WAVE_MAX : PATH_MAX_LABELS, NY = W / T, NONE = 0x7fffffff;
  __shared__ double f[PPB][W];
  __shared__ double red_v[4];
  __shared__ int red_i[4];
  const int team = threadIdx.x / T, t = threadIdx.x % T;
  const int64_t idx = (int64_t)blockIdx.x * PPB + team;
  if (idx >= count) return;          // (T == 64: a whole wave, and the wave form has no workgroup barrier; T == 256: never)
  const ForestNode nd = nodes[list[first + idx]];
  const PathNode pn{nd.dual_off, 0, 0, nd.d0, nd.factor, nd.link_begin, nd.n_links, -1, 0, 0, 0};
  const int64_t* ch = child_g + nd.child_begin;
  double* fv = f[team];
#pragma unroll
  for (int j = 0; j < NY; ++j) {
    const int x = t + j * T;
    if (x >= nd.d0) continue;
    double v = path_node_cost(pn, links, dual, cdata, primal, x, tab32);
    for (int c = 0; c < nd.n_children; ++c) v = v + rows[ch[c] + x];
    fv[x] = v;
  }
  path_sync<T>();
  if (nd.parent < 0) {
    // the first minimiser of f: per thread in ascending x, then value / index butterflies over the wave (and the waves)
    double bv = LPMP_INF; int bi = NONE;
#pragma unroll
    for (int j = 0; j < NY; ++j) { const int x = t + j * T; if (x < nd.d0 && (bi == NONE || fv[x] < bv)) { bv = fv[x]; bi = x; } }
    double mn = decode_min<64>(bv);
    int label = decode_min<64>((bi != NONE && bv == mn) ? bi : NONE);
    if (T > 64) {
      if ((threadIdx.x & 63) == 0) { red_v[threadIdx.x >> 6] = mn; red_i[threadIdx.x >> 6] = label; }
      __syncthreads();
      mn = LPMP_INF; label = NONE;
      for (int w = 0; w < T / 64; ++w)
        if (red_i[w] != NONE && (label == NONE || red_v[w] < mn || (red_v[w] == mn && red_i[w] < label))) { mn = red_v[w]; label = red_i[w]; }
    }
    if (t == 0) primal[2 * (int64_t)nd.factor] = label;
    return;
  }
#pragma unroll
  for (int j = 0; j < NY; ++j) {
    const int y = t + j * T;
    if (y >= nd.dq) continue;
    double g = LPMP_INF; int b = 0;
    switch (nd.edge_kind) {      // (uniform over the node's threads, as in path_moves_kernel)
      case LPMP_F_PAIRWISE_DENSE:
        if (tab32) path_min_plus<LPMP_F_PAIRWISE_DENSE, 1>(cdata, nd.edge_const, nd.edge_d1, nd.edge_side, fv, nd.d0, y, g, b);
        else path_min_plus<LPMP_F_PAIRWISE_DENSE, 0>(cdata, nd.edge_const, nd.edge_d1, nd.edge_side, fv, nd.d0, y, g, b);
        break;
      case LPMP_F_PAIRWISE_SHARED: path_min_plus<LPMP_F_PAIRWISE_SHARED, 0>(cdata, nd.edge_const, nd.edge_d1, nd.edge_side, fv, nd.d0, y, g, b); break;
      case LPMP_F_PAIRWISE_DIFF: path_min_plus<LPMP_F_PAIRWISE_DIFF, 0>(cdata, nd.edge_const, nd.edge_d1, nd.edge_side, fv, nd.d0, y, g, b); break;
      case LPMP_F_PAIRWISE_DIFF_SHIFT: path_min_plus<LPMP_F_PAIRWISE_DIFF_SHIFT, 0>(cdata, nd.edge_const, nd.edge_d1, nd.edge_side, fv, nd.d0, y, g, b); break;
      default: path_min_plus<LPMP_F_PAIRWISE_POTTS, 0>(cdata, nd.edge_const, nd.edge_d1, nd.edge_side, fv, nd.d0, y, g, b); break;
    }
    rows[nd.g_off + y] = g;
    if (nd.back_wide) reinterpret_cast<unsigned short*>(back + nd.back_off)[y] = (unsigned short)b;
    else back[nd.back_off + y] = (unsigned char)b;
  }
}
__global__ void __launch_bounds__(256)
forest_down_kernel(const int32_t* __restrict__ list, const ForestNode* __restrict__ nodes, int32_t* primal, const unsigned char* __restrict__ back,
                   int64_t first, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const ForestNode nd = nodes[list[first + i]];
  const int xq = primal[2 * (int64_t)nd.parent];     // (written by this group's up sweep or by the level above: inside [0, dq))
  primal[2 * (int64_t)nd.factor] = nd.back_wide ? (int)reinterpret_cast<const unsigned short*>(back + nd.back_off)[xq] : (int)back[nd.back_off + xq];
}

// LP::CheckPrimalConsistency (reference LP_MP.h:1067-1082): every message's two sides agree
__global__ void __launch_bounds__(256)
primal_check_kernel(const PrimalLink* __restrict__ links, int64_t n, const int32_t* __restrict__ primal, int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const PrimalLink l = links[i];
  if (primal[2 * (int64_t)l.u] != primal[2 * (int64_t)l.p + l.side]) *bad = 1;
}
// FactorContainer::EvaluatePrimal per factor: reparametrised cost at the factor's primal, +inf when a side is unset
__global__ void __launch_bounds__(256)
primal_cost_kernel(const LbRec* __restrict__ recs, const double* __restrict__ dual, const double* __restrict__ cdata,
                   const int32_t* __restrict__ primal, double* __restrict__ out, int64_t count, int tab32) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= count) return;
  const LbRec r = recs[f];
  const int kind = r.kind_flags & 15;
  const double* d = dual + r.dual_off;
  const int a = primal[2 * f], b = primal[2 * f + 1];
  double c;
  if (kind == LPMP_F_VECTOR) c = a < r.d0 ? d[a] : LPMP_INF;
  else if (a >= r.d0 || b >= r.d1) c = LPMP_INF;
  else c = pw_cost(cdata, r.const_off, kind, r.d1, a, b, tab32) + d[a] + d[r.d0 + b];
  out[f] = c;
}

// Table precision (engine.cpp): table k of the chunk — n doubles at src[src_off] — becomes n floats at dst[dst_off]; one wave
// per table.  An entry the mode refuses (strict: not exactly a float; both modes: a finite value that overflows float, a
// nonzero one below FLT_MIN) puts its factor into *bad, which keeps the lowest such index.  +-inf pass through.
__global__ void __launch_bounds__(256)
narrow_tables_kernel(const NarrowRec* __restrict__ recs, int64_t n, const double* __restrict__ src, float* __restrict__ dst, int strict,
                     int* __restrict__ bad) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * 4 + wave;
  if (k >= n) return;
  const NarrowRec r = recs[k];
  bool refuse = false;
  for (int64_t i = lane; i < r.n; i += 64) {
    const double x = src[r.src_off + i];
    const float f = (float)x;                     // round to nearest even
    const double ax = fabs(x);
    if (ax < LPMP_INF) {                          // finite (NaN: outside the contract, passes)
      if (fabsf(f) == __builtin_inff()) refuse = true;
      else if (x != 0.0 && ax < 1.17549435082228750797e-38) refuse = true;
      else if (strict && (double)f != x) refuse = true;
    }
    dst[r.dst_off + i] = f;
  }
  if (refuse) atomicMin(bad, r.factor);
}

// deterministic two-stage sum: block b sums a fixed contiguous slice in a fixed tree order
__global__ void __launch_bounds__(256)
sum_stage_kernel(const double* __restrict__ in, double* __restrict__ out, int64_t n, int64_t per_block) {
  __shared__ double sh[256];
  const int64_t b0 = (int64_t)blockIdx.x * per_block;
  const int64_t b1 = b0 + per_block < n ? b0 + per_block : n;
  double s = 0.0;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) s += in[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// counter-based generator of the synthetic workloads: bit-identical to lp_mp_amd.synthetic.u01
__global__ void synth_fill_kernel(double* __restrict__ out, int64_t n, uint64_t seed, uint64_t first) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uint64_t z = seed + (first + (uint64_t)i + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z = z ^ (z >> 31);
    out[i] = (double)(z >> 11) * (1.0 / 9007199254740992.0);
  }
}

// ---- launch wrappers (declared in kernels.hpp, called from engine.cpp) -----------------------------------------------------
void launch_sweep(int kclass, const UpdRec* recs, const Op* ops, double* dual, const double* cdata, const int32_t* tabs,
                  double* lb, int32_t* primal, const int32_t* pw_unary, int64_t first, int64_t count, int flags, hipStream_t s) {
  if (count <= 0) return;
  auto blocks = [&](int per_block) { return dim3((unsigned)((count + per_block - 1) / per_block)); };
  switch (kclass) {
    case KC_DENSE_BIG:
      if (flags & SWEEP_TAB32) {
        if (flags & SWEEP_NT) hipLaunchKernelGGL(sweep_dense_big_f32_kernel<true>, blocks(BIG_WAVES), dim3(64 * BIG_WAVES), big_lds_bytes(flags, 3), s, recs, ops, dual, cdata, lb, primal, first, count, flags);
        else hipLaunchKernelGGL(sweep_dense_big_f32_kernel<false>, blocks(BIG_WAVES), dim3(64 * BIG_WAVES), big_lds_bytes(flags, 3), s, recs, ops, dual, cdata, lb, primal, first, count, flags);
      } else
      if (flags & SWEEP_NT) hipLaunchKernelGGL(sweep_dense_big_kernel<true>, blocks(BIG_WAVES), dim3(64 * BIG_WAVES), big_lds_bytes(flags, 3), s, recs, ops, dual, cdata, lb, primal, first, count, flags);
      else hipLaunchKernelGGL(sweep_dense_big_kernel<false>, blocks(BIG_WAVES), dim3(64 * BIG_WAVES), big_lds_bytes(flags, 3), s, recs, ops, dual, cdata, lb, primal, first, count, flags);
      break;
    case KC_SMALL: hipLaunchKernelGGL(sweep_generic_kernel<1>, blocks(GenCtx<1>::FPB), dim3(GenCtx<1>::THREADS), 0, s, recs, ops, dual, cdata, tabs, lb, primal, pw_unary, first, count, flags); break;
    default: hipLaunchKernelGGL(sweep_generic_kernel<64>, blocks(GEN_WAVES), dim3(64 * GEN_WAVES), 0, s, recs, ops, dual, cdata, tabs, lb, primal, pw_unary, first, count, flags); break;
  }
}

// class KC_DIFF: one wave per record, dynamic LDS by the launch's label counts (flags: sweep_bigdim_flags)
void launch_sweep_diff(bool band, bool shift, const UpdRec* recs, const Op* ops, double* dual, const double* cdata, double* lb, int32_t* primal, int64_t first, int64_t count,
                       int flags, hipStream_t s) {
  if (count <= 0) return;
  if (band && shift) {                                 // a DIFF_SHIFT peer, every receive banded (LevelRange::diff_shift_band): LDS and waves of the banded kernel
    const int waves = big_waves(flags, DIFF_BAND_SLABS);
    hipLaunchKernelGGL(sweep_diff_shift_band_kernel, dim3((unsigned)((count + waves - 1) / waves)), dim3(64 * waves), big_lds_bytes(flags, DIFF_BAND_SLABS), s,
                       recs, ops, dual, cdata, lb, primal, first, count, flags);
    return;
  }
  if (band) {                                          // every receive of the launch has a banded D (LevelRange::diff_band)
    const int waves = big_waves(flags, DIFF_BAND_SLABS);
    hipLaunchKernelGGL(sweep_diff_band_kernel, dim3((unsigned)((count + waves - 1) / waves)), dim3(64 * waves), big_lds_bytes(flags, DIFF_BAND_SLABS), s,
                       recs, ops, dual, cdata, lb, primal, first, count, flags);
    return;
  }
  const int waves = big_waves(flags, DIFF_SLABS);
  if (shift) {                                         // a record of the launch has a DIFF_SHIFT peer (LevelRange::diff_shift): same LDS, same waves
    hipLaunchKernelGGL(sweep_diff_shift_kernel, dim3((unsigned)((count + waves - 1) / waves)), dim3(64 * waves), big_lds_bytes(flags, DIFF_SLABS), s,
                       recs, ops, dual, cdata, lb, primal, first, count, flags);
    return;
  }
  hipLaunchKernelGGL(sweep_diff_kernel, dim3((unsigned)((count + waves - 1) / waves)), dim3(64 * waves), big_lds_bytes(flags, DIFF_SLABS), s,
                     recs, ops, dual, cdata, lb, primal, first, count, flags);
}

// The ONE table kernel class -> template arguments of the packed kernels: f(family, integral_constant<int, L>, bool_constant<VAR>)
// for a class that has a label width L (VAR: its run-time-dims form), and f's answer; false for every other class.  A wrapper
// instantiates a kernel only in the `if constexpr` branch of the families it serves, so the kernels that exist are exactly
// the ones its branches name.
enum Family { FAM_DENSE, FAM_POTTS, FAM_PW, FAM_SHARED };
template <Family F, bool VAR, class Fn>
static bool with_width(int width, Fn&& f) {
  using Fam = std::integral_constant<Family, F>;
  switch (width) {
    case 32: return f(Fam{}, std::integral_constant<int, 32>{}, std::bool_constant<VAR>{});
    case 16: return f(Fam{}, std::integral_constant<int, 16>{}, std::bool_constant<VAR>{});
    case 8: return f(Fam{}, std::integral_constant<int, 8>{}, std::bool_constant<VAR>{});
    case 4: return f(Fam{}, std::integral_constant<int, 4>{}, std::bool_constant<VAR>{});
    default: return false;
  }
}
template <class Fn>
static bool with_class(int kclass, Fn&& f) {
  const int w = kc_width(kclass);
  if (kclass >= KC_DENSE_4 && kclass <= KC_DENSE_32) return with_width<FAM_DENSE, false>(w, f);
  if (kclass >= KC_POTTS_4 && kclass <= KC_POTTS_32) return with_width<FAM_POTTS, false>(w, f);
  if (kclass >= KC_DENSE_V4 && kclass <= KC_DENSE_V32) return with_width<FAM_DENSE, true>(w, f);
  if (kclass >= KC_POTTS_V4 && kclass <= KC_POTTS_V32) return with_width<FAM_POTTS, true>(w, f);
  if (kc_is_pw(kclass)) return with_width<FAM_PW, false>(w, f);
  if (kc_is_shared(kclass)) return with_width<FAM_SHARED, true>(w, f);   // (dims from the table descriptors)
  return false;
}
// receives in flight per lane group of the dense kernels: 2 at 16 / 32 labels (1 and 4 measured slower on C3), 4 below
constexpr int recv_in_flight(int L) { return L >= 16 ? 2 : 4; }

// compute units of the CURRENT device (a process may hold engines on several devices): asked once, cached per device ordinal
// (engines on several host threads share the cache: relaxed atomics, every thread would store the same value).  di: the cache slot.
static int device_cu_count(int& di) {
  static std::atomic<int> n_cu_of[64];
  int dev = 0; (void)hipGetDevice(&dev);
  di = dev >= 0 && dev < 64 ? dev : 0;
  int n_cu = n_cu_of[di].load(std::memory_order_relaxed);
  if (n_cu == 0) { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256; n_cu = v; n_cu_of[di].store(v, std::memory_order_relaxed); }
  return n_cu;
}

// Returns false when the class has no packed kernel for the request: an unknown class, and on the pairwise classes the
// residual rule or a launch without packets (stride <= 0).
bool launch_sweep_packed(int kclass, const Op* packets, const UpdRec* recs, const Op* ops, int stride, double* dual, const double* cdata,
                         double* lb, int32_t* primal, int64_t count, int flags, hipStream_t s) {
  if (count <= 0) return true;
  auto blocks = [&](int per_block) { return dim3((unsigned)((count + per_block - 1) / per_block)); };
  const bool nt = (flags & SWEEP_NT) != 0, t32 = (flags & SWEEP_TAB32) != 0;
  return with_class(kclass, [&](auto fam, auto width, auto var) {
    constexpr Family F = decltype(fam)::value; constexpr int L = decltype(width)::value; constexpr bool VAR = decltype(var)::value;
    if constexpr (F == FAM_PW) {
      // (the residual rule recomputes the min-marginals after every send: the op-by-op generic kernel does that)
      if ((flags & SWEEP_RESIDUAL) || stride <= 0) return false;
      if (t32) hipLaunchKernelGGL((sweep_pairwise_pk_f32_kernel<L>), blocks(256 / DenseCfg<L>::G), dim3(256), 0, s, packets, dual, cdata, lb, count, stride);
      else hipLaunchKernelGGL((sweep_pairwise_pk_kernel<L>), blocks(256 / DenseCfg<L>::G), dim3(256), 0, s, packets, dual, cdata, lb, count, stride);
      return true;
    } else if constexpr (F == FAM_DENSE) {
      constexpr int K = recv_in_flight(L);
      if (t32) {   // float tables: the same choice among the f32 kernels
        if constexpr (!VAR) if (nt) { hipLaunchKernelGGL((sweep_dense_pk_f32_kernel<L, K, false, true>), blocks(256 / DenseCfg<L>::G), dim3(256), 0, s, packets, recs, ops, dual, cdata, lb, primal, count, stride, flags); return true; }
        hipLaunchKernelGGL((sweep_dense_pk_f32_kernel<L, K, VAR, false>), blocks(256 / DenseCfg<L>::G), dim3(256), 0, s, packets, recs, ops, dual, cdata, lb, primal, count, stride, flags);
        return true;
      }
      // (run-time dims: rows are not line-aligned, consecutive 8-B loads share lines — non-temporal loads cost 9 % there)
      if constexpr (!VAR) if (nt) { hipLaunchKernelGGL((sweep_dense_pk_kernel<L, K, false, true>), blocks(256 / DenseCfg<L>::G), dim3(256), 0, s, packets, recs, ops, dual, cdata, lb, primal, count, stride, flags); return true; }
      hipLaunchKernelGGL((sweep_dense_pk_kernel<L, K, VAR, false>), blocks(256 / DenseCfg<L>::G), dim3(256), 0, s, packets, recs, ops, dual, cdata, lb, primal, count, stride, flags);
      return true;
    } else if constexpr (F == FAM_POTTS) {
      if constexpr (!VAR) if (nt) { hipLaunchKernelGGL((sweep_potts_pk_kernel<L, false, true>), blocks(256 / L), dim3(256), 0, s, packets, recs, ops, dual, cdata, lb, primal, count, stride, flags); return true; }
      hipLaunchKernelGGL((sweep_potts_pk_kernel<L, VAR, false>), blocks(256 / L), dim3(256), 0, s, packets, recs, ops, dual, cdata, lb, primal, count, stride, flags);
      return true;
    } else return false;   // (the shared classes: launch_sweep_shared)
  });
}

// shared classes: a persistent grid (what is resident at once, at most one workgroup per block of records); dynamic LDS = the
// launch's table slots.  tabs = n_tabs indices into the pool described by desc (device array, engine.cpp).
template <int L, bool NT>
static void launch_shared_one(const Op* packets, const UpdRec* recs, const Op* ops, int stride, double* dual, const double* cdata, double* lb,
                              int32_t* primal, int64_t count, int flags, const ShTableDesc* desc, const ShTabList& list, hipStream_t s) {
  auto k = sweep_shared_pk_kernel<L, NT>;
  const size_t lds = (size_t)2 * (list.n > 0 ? list.n : 1) * L * L * sizeof(double);
  // resident workgroups per CU by table count: asked once, cached like the CU count
  static std::atomic<int> per_cu_of[64][SHARED_MAX_TABLES + 1];
  int di = 0;
  const int n_cu = device_cu_count(di), ti = list.n > 0 && list.n <= SHARED_MAX_TABLES ? list.n : 0;
  int per_cu = per_cu_of[di][ti].load(std::memory_order_relaxed);
  if (per_cu == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, 256, lds) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 1; }
    per_cu_of[di][ti].store(per_cu, std::memory_order_relaxed);
  }
  constexpr int GPB = 256 / DenseCfg<L>::G;
  const int64_t n_blocks = (count + GPB - 1) / GPB, cap = (int64_t)n_cu * per_cu;
  hipLaunchKernelGGL(k, dim3((unsigned)(n_blocks < cap ? n_blocks : cap)), dim3(256), lds, s, packets, recs, ops, dual, cdata, lb, primal, count, stride, flags, desc, list);
}
// Returns false for a class that is not a shared one, a launch without packets or indirect records (stride == 0), a table count out of
// range or no descriptors.
bool launch_sweep_shared(int kclass, const Op* packets, const UpdRec* recs, const Op* ops, int stride, double* dual, const double* cdata,
                         double* lb, int32_t* primal, int64_t count, int flags, const ShTableDesc* desc, const int32_t* tabs, int n_tabs, hipStream_t s) {
  if (count <= 0) return true;
  if (!kc_is_shared(kclass) || stride == 0 || n_tabs < 0 || n_tabs > SHARED_MAX_TABLES || !desc) return false;
  ShTabList list; list.n = n_tabs;
  for (int q = 0; q < SHARED_MAX_TABLES; ++q) list.t[q] = q < n_tabs ? tabs[q] : 0;
  const bool nt = (flags & SWEEP_NT) != 0;
  return with_class(kclass, [&](auto fam, auto width, auto) {
    if constexpr (decltype(fam)::value == FAM_SHARED) {
      constexpr int L = decltype(width)::value;
      if (nt) launch_shared_one<L, true>(packets, recs, ops, stride, dual, cdata, lb, primal, count, flags, desc, list, s);
      else launch_shared_one<L, false>(packets, recs, ops, stride, dual, cdata, lb, primal, count, flags, desc, list, s);
      return true;
    } else return false;
  });
}

// chain executor: one persistent launch for a deep single-class schedule; grid = what is resident at once (more
// workgroups would only queue behind the running ones).  Returns false for a class without a chain kernel.
template <class K>
static unsigned chain_grid(K kernel, int n_tickets, int threads = 256, int* per_cu_out = nullptr, int max_wgs = 0) {
  int di = 0;
  const int n_cu = device_cu_count(di);
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  if (per_cu_out) *per_cu_out = per_cu;
  long cap = (long)n_cu * per_cu;
  if (max_wgs > 0 && max_wgs < cap) cap = max_wgs;
  return (unsigned)(n_tickets < cap ? n_tickets : cap);
}
// what launch_chain will launch for a peer-minima chain of n_tickets (LPMP_ROT_VERBOSE, engine.cpp)
template <class F>
static auto with_pq_kernel(int pq_lds, int pq_hold, bool wide, bool scatter, F f) {
  if (pq_lds != 0 && pq_hold == 3 && scatter) return wide ? f(chain_dense_pq_scatter_kernel<32, 32>) : f(chain_dense_pq_scatter_kernel<32, 64>);
  if (pq_lds != 0 && pq_hold == 3) return wide ? f(chain_dense_pq_kernel<32, 3, 1, 32>) : f(chain_dense_pq_kernel<32, 3, 1>);
  if (wide) return pq_lds == 0 ? f(chain_dense_pq_kernel<32, PQ_KM, 0, 32>) : f(chain_dense_pq_kernel<32, PQ_KM, 1, 32>);
  return pq_lds == 0 ? f(chain_dense_pq_kernel<32, PQ_KM>) : f(chain_dense_pq_kernel<32, PQ_KM, 1>);
}
unsigned chain_pq_grid(int pq_lds, int pq_hold, bool pq_wide, bool pq_scatter, int n_tickets, int* per_cu, int* num_regs, int* scratch_bytes, int pq_ahead, int max_wgs) {
  auto report = [&](auto k) {
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k)) != hipSuccess) { (void)hipGetLastError(); fa.numRegs = -1; fa.localSizeBytes = (size_t)-1; }
    if (num_regs) *num_regs = fa.numRegs;
    if (scratch_bytes) *scratch_bytes = (int)fa.localSizeBytes;
    return chain_grid(k, n_tickets, 256, per_cu, max_wgs);
  };
  if (pq_ahead != 0 && pq_ahead_applies(pq_lds, pq_hold, pq_wide, pq_scatter, 0)) return pq_ahead == 2 ? report(chain_dense_pq_ahead_kernel<32, 32, false>) : report(chain_dense_pq_ahead_kernel<32, 32, true>);
  return with_pq_kernel(pq_lds, pq_hold, pq_wide, pq_scatter, report);
}
void debug_set_level_trace(long long* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_level_trace), &p, sizeof(p)); }
bool launch_level_loop(int kclass, int flags, const ChainLaunch* ln, int n_launches, double* dual, const double* cdata,
                       const int32_t* tabs, double* lb, hipStream_t s) {
  if (kclass == KC_SMALL) hipLaunchKernelGGL(level_loop_kernel<1>, dim3(1), dim3(64 * (LL_WAVES + 1)), 0, s, ln, n_launches, dual, cdata, tabs, lb, flags);
  else if (kclass == KC_GENERIC) hipLaunchKernelGGL(level_loop_kernel<64>, dim3(1), dim3(GenCtx<64>::THREADS), 0, s, ln, n_launches, dual, cdata, tabs, lb, flags);
  else return false;
  return true;
}
bool launch_chain(int kclass, int flags, const ChainArgs& ca, const ChainLaunch* ln, double* dual, const double* cdata,
                  const int32_t* tabs, double* lb, int32_t* primal, hipStream_t s, double* peerq, int pq_lds, bool pq_wide, int pq_hold, bool pq_scatter,
                  const ChainAhead& ahead, int max_wgs) {
  const bool nt = (flags & SWEEP_NT) != 0, mailbox = ca.mailbox != nullptr, t32 = (flags & SWEEP_TAB32) != 0;
  if (peerq) {   // joined passes with peer minima: no other class, table format or send rule has the form
    if (kclass != KC_DENSE_32 || flags != 0 || mailbox) return false;
    if (ahead.form != 0) {   // (the engine asks for it only where it applies)
      if (!ahead.desc || !pq_ahead_applies(pq_lds, pq_hold, pq_wide, pq_scatter, ahead.n_launches)) return false;
      auto k = ahead.form == 2 ? chain_dense_pq_ahead_kernel<32, 32, false> : chain_dense_pq_ahead_kernel<32, 32, true>;
      hipLaunchKernelGGL(k, dim3(chain_grid(k, ca.n_tickets, 256, nullptr, max_wgs)), dim3(256), 0, s, ca, ahead, ln, dual, cdata, lb, peerq);
      return true;
    }
    auto go = [&](auto k) { hipLaunchKernelGGL(k, dim3(chain_grid(k, ca.n_tickets, 256, nullptr, max_wgs)), dim3(256), 0, s, ca, ln, dual, cdata, lb, peerq); return true; };
    return with_pq_kernel(pq_lds, pq_hold, pq_wide, pq_scatter, go);
  }
  auto packed = [&](auto k) { hipLaunchKernelGGL(k, dim3(chain_grid(k, ca.n_tickets, 256, nullptr, max_wgs)), dim3(256), 0, s, ca, ln, dual, cdata, lb, primal, flags); return true; };
  auto generic = [&](auto k, int threads) { hipLaunchKernelGGL(k, dim3(chain_grid(k, ca.n_tickets, threads, nullptr, max_wgs)), dim3(threads), 0, s, ca, ln, dual, cdata, tabs, lb, flags); return true; };
  if (kclass == KC_GENERIC) return generic(chain_generic_kernel<64>, GenCtx<64>::THREADS);
  if (kclass == KC_SMALL) return generic(chain_generic_kernel<1>, GenCtx<1>::THREADS);
  return with_class(kclass, [&](auto fam, auto width, auto var) {
    constexpr Family F = decltype(fam)::value; constexpr int L = decltype(width)::value; constexpr bool VAR = decltype(var)::value;
    // the mailbox form is an instantiation of its own (the joined passes of the headline grid lost 8 % with the mailbox fields in
    // their registers: dense_pk_body), and a mailbox chain is a deep schedule: latency-bound, no streaming variant; the
    // run-time-dims forms have none either (launch_sweep_packed)
    if constexpr (F == FAM_DENSE) {
      constexpr int K = recv_in_flight(L);
      if (t32) {
        if (mailbox) return packed(chain_dense_pk_f32_kernel<L, K, VAR, false, true>);
        if constexpr (!VAR) if (nt) return packed(chain_dense_pk_f32_kernel<L, K, false, true, false>);
        return packed(chain_dense_pk_f32_kernel<L, K, VAR, false, false>);
      }
      if (mailbox) return packed(chain_dense_pk_kernel<L, K, VAR, false, true>);
      if constexpr (!VAR) if (nt) return packed(chain_dense_pk_kernel<L, K, false, true, false>);
      return packed(chain_dense_pk_kernel<L, K, VAR, false, false>);
    } else if constexpr (F == FAM_POTTS) {
      return mailbox ? packed(chain_potts_pk_kernel<L, VAR, true>) : packed(chain_potts_pk_kernel<L, VAR, false>);
    } else return false;   // (pairwise and shared classes have no chain form: kc_chain_capable)
  });
}

void launch_factor_lb(const LbRec* recs, const double* dual, const double* cdata, double* out, int64_t count, int tab32, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(factor_lb_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, recs, dual, cdata, out, count, tab32);
}

// the streaming bound of square dense factors of 8 / 16 / 32 labels; false for every other L
bool launch_dense_lb(int L, const LbRec* recs, const double* dual, const double* cdata, double* out, int64_t first, int64_t count, int tab32, hipStream_t s) {
  if (count <= 0) return true;
  return with_width<FAM_DENSE, false>(L, [&](auto, auto width, auto) {
    constexpr int W = decltype(width)::value;
    if constexpr (W >= 8) {
      constexpr int per_block = 256 / DenseCfg<W>::G;
      hipLaunchKernelGGL(dense_lb_kernel<W>, dim3((unsigned)((count + per_block - 1) / per_block)), dim3(256), 0, s, recs, dual, cdata, out, first, count, tab32);
      return true;
    } else return false;
  });
}

void launch_lb_collect_stale(const double* lb, int64_t n, int32_t* list, unsigned long long* counter, hipStream_t s) {
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(lb_collect_stale_kernel, dim3((unsigned)blocks), dim3(256), 0, s, lb, n, list, counter);
}
void launch_factor_lb_list(const LbRec* recs, const double* dual, const double* cdata, double* out, const int32_t* list, int64_t count, int tab32, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(factor_lb_list_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, recs, dual, cdata, out, list, count, tab32);
}

static dim3 blocks256(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }
void launch_primal_init(const PrimalInit* list, int64_t n, int32_t* primal, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(primal_init_kernel, blocks256(n), dim3(256), 0, s, list, n, primal);
}
void launch_primal_propagate(const PrimalLink* links, int64_t n, int32_t* primal, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(primal_propagate_kernel, blocks256(n), dim3(256), 0, s, links, n, primal);
}
template <int G, int CH>
static void launch_decode_as(const DecodeRec* recs, const DecodeLink* links, const double* dual, const double* cdata, int32_t* primal,
                             int64_t first, int64_t count, int level, int flags, int tab32, hipStream_t s) {
  constexpr int GPB = 256 / G;
  hipLaunchKernelGGL((decode_kernel<G, CH>), dim3((unsigned)((count + GPB - 1) / GPB)), dim3(256), 0, s, recs, links, dual, cdata, primal, first, count,
                     level, flags, tab32);
}
void launch_path_moves(const PathRec* paths, const PathNode* nodes, const PathLink* links, const double* dual, const double* cdata,
                       int32_t* primal, unsigned char* back, int64_t first, int64_t count, int wide, int tab32, hipStream_t s) {
  if (count <= 0) return;
  if (wide) hipLaunchKernelGGL((path_moves_kernel<256>), dim3((unsigned)count), dim3(256), 0, s, paths, nodes, links, dual, cdata, primal, back, first, count, tab32);
  else hipLaunchKernelGGL((path_moves_kernel<64>), dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, paths, nodes, links, dual, cdata, primal, back, first, count, tab32);
}
void launch_forest_up(const int32_t* list, const ForestNode* nodes, const int64_t* child_g, const PathLink* links, const double* dual, const double* cdata,
                      int32_t* primal, double* rows, unsigned char* back, int64_t first, int64_t count, int wide, int tab32, hipStream_t s) {
  if (count <= 0) return;
  if (wide) hipLaunchKernelGGL((forest_up_kernel<256>), dim3((unsigned)count), dim3(256), 0, s, list, nodes, child_g, links, dual, cdata, primal, rows, back, first, count, tab32);
  else hipLaunchKernelGGL((forest_up_kernel<64>), dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, list, nodes, child_g, links, dual, cdata, primal, rows, back, first, count, tab32);
}
void launch_forest_down(const int32_t* list, const ForestNode* nodes, int32_t* primal, const unsigned char* back, int64_t first, int64_t count, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(forest_down_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, list, nodes, primal, back, first, count);
}
void launch_decode(const DecodeRec* recs, const DecodeLink* links, const double* dual, const double* cdata, int32_t* primal,
                   int64_t first, int64_t count, int width, int level, int flags, int tab32, hipStream_t s) {
  if (count <= 0) return;
  if (width <= 4) launch_decode_as<4, 1>(recs, links, dual, cdata, primal, first, count, level, flags, tab32, s);
  else if (width <= 8) launch_decode_as<8, 1>(recs, links, dual, cdata, primal, first, count, level, flags, tab32, s);
  else if (width <= 16) launch_decode_as<16, 1>(recs, links, dual, cdata, primal, first, count, level, flags, tab32, s);
  else if (width <= DECODE_GROUP_MAX) launch_decode_as<32, 1>(recs, links, dual, cdata, primal, first, count, level, flags, tab32, s);
  else if (width <= 64) launch_decode_as<64, 1>(recs, links, dual, cdata, primal, first, count, level, flags, tab32, s);
  else launch_decode_as<64, DECODE_CHUNK / 64>(recs, links, dual, cdata, primal, first, count, level, flags, tab32, s);
}
void launch_primal_check(const PrimalLink* links, int64_t n, const int32_t* primal, int* bad, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(primal_check_kernel, blocks256(n), dim3(256), 0, s, links, n, primal, bad);
}
void launch_primal_cost(const LbRec* recs, const double* dual, const double* cdata, const int32_t* primal, double* out, int64_t count, int tab32, hipStream_t s) {
  if (count > 0) hipLaunchKernelGGL(primal_cost_kernel, blocks256(count), dim3(256), 0, s, recs, dual, cdata, primal, out, count, tab32);
}

// ---- rows layout (engine.cpp): a dense pairwise factor's table and its two message vectors in ONE contiguous row ----------
// [T (d0 x d1) | m1 (d0) | m2 (d1)] of an engine-private buffer, so that a receive's three reads are one burst (a random
// graph's receives otherwise touch a 2-KiB table and two single 128-byte lines somewhere else: C4).  The packed
// arrays stay the boundary's format (serialize_dual order); these copies move between the two.
//   what 0: build a row (table from the packed constants, vectors from the packed duals)
//   what 1: packed duals -> rows (vectors only)      what 2: rows -> packed duals (vectors only)
__global__ void __launch_bounds__(256)
rows_copy_kernel(const RowRec* __restrict__ recs, int64_t n, const double* __restrict__ cdata, double* __restrict__ dual, double* __restrict__ rows, int what) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  if (i >= n) return;
  const RowRec r = recs[i];
  const int nt = r.d0 * r.d1, nm = r.d0 + r.d1;
  double* row = rows + r.row_off;
  if (what == 0) for (int x = lane; x < nt; x += 64) row[x] = cdata[r.const_off + x];
  if (what == 2) { for (int x = lane; x < nm; x += 64) dual[r.dual_off + x] = row[nt + x]; }
  else { for (int x = lane; x < nm; x += 64) row[nt + x] = dual[r.dual_off + x]; }
}
// Device placement of the SHARED factors' constants (engine.cpp): cell k arrives as {packed const offset of the factor (int64),
// table offset relative to the const base (int64)} and becomes {scale read from the packed constants, table offset}
__global__ void __launch_bounds__(256)
shared_cells_kernel(double* __restrict__ cells, int64_t n, const double* __restrict__ cdata) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int64_t coff = __double_as_longlong(cells[2 * k]);
  cells[2 * k] = cdata[coff];
}
void launch_shared_cells(double* cells, int64_t n, const double* cdata, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(shared_cells_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cells, n, cdata);
}

void launch_rows_copy(const RowRec* recs, int64_t n, const double* cdata, double* dual, double* rows, int what, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(rows_copy_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, recs, n, cdata, dual, rows, what);
}

void launch_narrow_tables(const NarrowRec* recs, int64_t n, const double* src, float* dst, int strict, int* bad, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(narrow_tables_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, recs, n, src, dst, strict, bad);
}

void launch_sum_stage(const double* in, double* out, int64_t n, int64_t per_block, int64_t n_blocks, hipStream_t s) {
  hipLaunchKernelGGL(sum_stage_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, in, out, n, per_block);
}

void launch_synth_fill(double* out, int64_t n, uint64_t seed, uint64_t first, hipStream_t s) {
  if (n <= 0) return;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(synth_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, n, seed, first);
}

// ---- new costs on a planned model (engine.cpp, lpmp_set_vectors / lpmp_zero_pairwise_duals) -----------------------------
// Both are streams: no LDS, no atomics, plain 8-byte loads and stores; consecutive lanes touch consecutive doubles.
// theta of listed vector factor k := (accumulate: +=, one IEEE add per entry) row src_row of src; one wave per record, lanes
// stride over the entries.  The factor's tracked bound becomes NaN: the next lower bound recomputes exactly these.
__global__ void __launch_bounds__(256)
set_vectors_kernel(const SetVecRec* __restrict__ recs, int64_t n, const double* __restrict__ src, int64_t src_stride, double* __restrict__ dual,
                   double* __restrict__ lb, int accumulate) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * 4 + wave;
  if (k >= n) return;
  const SetVecRec r = recs[k];
  const double* row = src + r.src_row * src_stride;
  double* th = dual + r.dual_off;
  if (accumulate) { for (int x = lane; x < r.len; x += 64) th[x] = th[x] + row[x]; }
  else { for (int x = lane; x < r.len; x += 64) th[x] = row[x]; }
  if (lane == 0) lb[r.factor] = __longlong_as_double(-1LL);   // all bits set: the NaN the stale marks of the sweep kernels are
}
// the message vectors of the pairwise factors := +0.0: runs of (device dual offset, length), merged by the host where they are
// contiguous and cut into pieces of at most ZERO_RUN_MAX doubles; one wave per piece, as set_vectors_kernel — where nothing merges
// (rows layout, pairwise factors between vectors) a piece is one factor's d0 + d1 doubles and no lane of a wider block would idle
__global__ void __launch_bounds__(256)
zero_pairwise_kernel(const ZeroRec* __restrict__ recs, int64_t n, double* __restrict__ dual) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * 4 + wave;
  if (k >= n) return;
  const ZeroRec r = recs[k];
  double* d = dual + r.dual_off;
  for (int64_t x = lane; x < r.len; x += 64) d[x] = 0.0;
}
// constants of listed pairwise factor k := row src_row of src (engine.cpp, lpmp_set_constants): one wave per record, lanes stride over
// the entries, 64-bit offsets (a table may start past 2^32 doubles).  A record names every place the sweep kernels read the
// factor's constants from — the Potts scalar; the first word of a SHARED / DIFF cell (of both cells of a DIFF_SHIFT factor) and the scalar the cell was gathered from; a
// dense table in the packed constants and in the factor's row of the rows layout; or the float table, narrowed here as
// narrow_tables_kernel narrows (round to nearest even).  The check kernel applies that kernel's refusals to the rows of the float
// tables and writes nothing else: the host launches it first and stops before any store when a row is refused.
__device__ __forceinline__ bool narrow_refuses(double x, int strict) {
  const float f = (float)x;
  const double ax = fabs(x);
  if (!(ax < LPMP_INF)) return false;              // +-inf pass through (NaN: outside the contract, passes)
  if (fabsf(f) == __builtin_inff()) return true;
  if (x != 0.0 && ax < 1.17549435082228750797e-38) return true;
  return strict && (double)f != x;
}
__global__ void __launch_bounds__(256)
set_constants_check_kernel(const SetConstRec* __restrict__ recs, int64_t n, const double* __restrict__ src, int64_t src_stride, int strict,
                           int* __restrict__ bad) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * 4 + wave;
  if (k >= n) return;
  const SetConstRec r = recs[k];
  if (!r.f32) return;
  const double* row = src + r.src_row * src_stride;
  bool refuse = false;
  for (int x = lane; x < r.len; x += 64) refuse = refuse || narrow_refuses(row[x], strict);
  if (refuse) atomicMin(bad, r.factor);
}
__global__ void __launch_bounds__(256)
set_constants_kernel(const SetConstRec* __restrict__ recs, int64_t n, const double* __restrict__ src, int64_t src_stride, double* __restrict__ cdata,
                     double* __restrict__ lb) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * 4 + wave;
  if (k >= n) return;
  const SetConstRec r = recs[k];
  const double* row = src + r.src_row * src_stride;
  if (r.f32) {
    float* t = reinterpret_cast<float*>(cdata + r.dst);
    for (int x = lane; x < r.len; x += 64) t[x] = (float)row[x];
  } else {
    double* a = cdata + r.dst;
    const int step = r.two == 2 ? 2 : 1;               // (two == 2, a DIFF_SHIFT factor: the first words of its two cells, and the two scalars)
    for (int x = lane; x < r.len; x += 64) a[step * x] = row[x];
    if (r.two) { double* b = cdata + r.dst2; for (int x = lane; x < r.len; x += 64) b[x] = row[x]; }
  }
  if (lane == 0) lb[r.factor] = __longlong_as_double(-1LL);   // stale, as set_vectors_kernel marks it
}
void launch_set_constants_check(const SetConstRec* recs, int64_t n, const double* src, int64_t src_stride, int strict, int* bad, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(set_constants_check_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, recs, n, src, src_stride, strict, bad);
}
void launch_set_constants(const SetConstRec* recs, int64_t n, const double* src, int64_t src_stride, double* cdata, double* lb, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(set_constants_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, recs, n, src, src_stride, cdata, lb);
}
void launch_set_vectors(const SetVecRec* recs, int64_t n, const double* src, int64_t src_stride, double* dual, double* lb, int accumulate, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(set_vectors_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, recs, n, src, src_stride, dual, lb, accumulate);
}
void launch_zero_pairwise(const ZeroRec* recs, int64_t n, double* dual, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(zero_pairwise_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, recs, n, dual);
}

// ---- prepared read-outs (prepared.cpp, lpmp_readout_*) ----------------------------------------------------------
// Gathers over a device record list into the caller's array: no LDS, no atomics, plain vector stores, 64-bit offsets.  Nothing but
// dst is written, and of a row only the entries below the factor's label count.
// labels: one thread per listed factor; dst[i] = its label slot of the primal array
__global__ void __launch_bounds__(256)
readout_labels_kernel(const ReadoutRec* __restrict__ recs, int64_t n, const int32_t* __restrict__ primal, int32_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const ReadoutRec r = recs[i];
  dst[r.row] = primal[2 * (int64_t)r.factor];
}
// vectors: G lanes per listed factor stride over its theta; consecutive lanes write consecutive doubles of the row
template <int G>
__global__ void __launch_bounds__(256)
readout_vectors_kernel(const ReadoutRec* __restrict__ recs, int64_t n, const double* __restrict__ dual, double* __restrict__ dst, int64_t dst_stride) {
  constexpr int GPB = 256 / G;
  const int grp = threadIdx.x / G, g = threadIdx.x % G;
  const int64_t i = (int64_t)blockIdx.x * GPB + grp;
  if (i >= n) return;
  const ReadoutRec r = recs[i];
  const double* th = dual + r.dual_off;
  double* row = dst + r.row * dst_stride;
  for (int x = g; x < r.d0; x += G) row[x] = th[x];
}
// beliefs: per-label min-marginal estimates of a unary u,
//   b[x] = theta_u[x];  for every link k of u in the order of its message list:  b[x] = b[x] + (m_s[x] + q[x]),
//   q[x] = min_y (cost_p(x, y) + m_o[y]) when u is on side 0 of pairwise factor p, cost_p(y, x) on side 1
// — what the receive phase of a sweep leaves in theta_u when u receives over all its messages and sends nothing.  G lanes per
// unary, a lane holds CH entries of b (x = base + j * G + g); a unary of more than G * CH labels is done chunk by chunk, the links
// read again.  Per link the table is read line by line, every line contiguous over the lanes:
//   side 1 (u indexes the columns): the lanes hold x and walk the rows y; m_o[y] is one load per group and row
//   side 0 (u indexes the rows):    the lanes hold y (strided when the peer has more labels than the group lanes), one row x per step,
//                                   a group minimum per row that the lane holding x keeps
// The next link's record, its m_s and the first stride of its m_o are requested before the current table is reduced.
template <int G, int CH>
struct BeliefFetch {
  DecodeLink lk; double ms[CH]; double mo0; bool have;
  __device__ __forceinline__ void load(const DecodeLink* __restrict__ links, int k, int n, const double* __restrict__ dual, int base, int g, int d0) {
    have = k < n;
    if (!have) return;
    lk = links[k];
    const double* m = dual + lk.peer_dual;
    const double* own = m + (lk.side ? lk.pd0 : 0);
#pragma unroll
    for (int j = 0; j < CH; ++j) { const int x = base + j * G + g; ms[j] = x < d0 ? own[x] : 0.0; }
    mo0 = (lk.side == 0 && g < lk.pd1) ? m[lk.pd0 + g] : LPMP_INF;
  }
};
template <int G, int CH>
__global__ void __launch_bounds__(256)
readout_beliefs_kernel(const ReadoutRec* __restrict__ recs, const DecodeLink* __restrict__ links, const double* __restrict__ dual,
                       const double* __restrict__ cdata, double* __restrict__ dst, int64_t dst_stride, int64_t first, int64_t count, int tab32) {
  constexpr int GPB = 256 / G;
  const int grp = threadIdx.x / G, g = threadIdx.x % G;
  const int64_t idx = (int64_t)blockIdx.x * GPB + grp;
  const bool live = idx < count;
  ReadoutRec r;
  if (live) r = recs[first + idx]; else { r.dual_off = 0; r.row = 0; r.d0 = 0; r.factor = 0; r.link_begin = 0; r.n_links = 0; }
  const int d0 = r.d0, n = r.n_links;
  const DecodeLink* lks = links + r.link_begin;
  const double* th = dual + r.dual_off;
  double* row = dst + r.row * dst_stride;
  for (int base = 0; base < d0; base += G * CH) {
    double b[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) { const int x = base + j * G + g; b[j] = x < d0 ? th[x] : 0.0; }
    BeliefFetch<G, CH> cur, nxt;
    cur.load(lks, 0, n, dual, base, g, d0);
    for (int k = 0; k < n; ++k) {
      nxt.load(lks, k + 1, n, dual, base, g, d0);
      const DecodeLink& lk = cur.lk;
      const double* m = dual + lk.peer_dual;
      double q[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j) q[j] = LPMP_INF;
      if (lk.side) {
        for (int y = 0; y < lk.pd0; ++y) {
          const double mo = m[y];
#pragma unroll
          for (int j = 0; j < CH; ++j) {
            const int x = base + j * G + g;
            if (x < d0) q[j] = fmin(q[j], pw_cost(cdata, lk.peer_const, lk.kind, lk.pd1, y, x, tab32) + mo);
          }
        }
      } else {
        const int od = lk.pd1;
        const double* mo = m + lk.pd0;
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int end = min(G, d0 - (base + j * G));        // rows of this stride (the same for every lane of the group)
          for (int xx = 0; xx < end; ++xx) {
            const int x = base + j * G + xx;
            double v = LPMP_INF;
            if (g < od) v = pw_cost(cdata, lk.peer_const, lk.kind, od, x, g, tab32) + cur.mo0;
            for (int y = g + G; y < od; y += G) v = fmin(v, pw_cost(cdata, lk.peer_const, lk.kind, od, x, y, tab32) + mo[y]);
            v = vec_min<G, G>(v);
            if (g == xx) q[j] = v;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < CH; ++j) b[j] = b[j] + (cur.ms[j] + q[j]);
      cur = nxt;
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) { const int x = base + j * G + g; if (x < d0) row[x] = b[j]; }
  }
}
void launch_readout_labels(const ReadoutRec* recs, int64_t n, const int32_t* primal, int32_t* dst, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(readout_labels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, recs, n, primal, dst);
}
template <int G>
static void launch_readout_vectors_as(const ReadoutRec* recs, int64_t n, const double* dual, double* dst, int64_t dst_stride, hipStream_t s) {
  constexpr int GPB = 256 / G;
  hipLaunchKernelGGL((readout_vectors_kernel<G>), dim3((unsigned)((n + GPB - 1) / GPB)), dim3(256), 0, s, recs, n, dual, dst, dst_stride);
}
void launch_readout_vectors(const ReadoutRec* recs, int64_t n, int width, const double* dual, double* dst, int64_t dst_stride, hipStream_t s) {
  if (n <= 0) return;
  if (width <= 8) launch_readout_vectors_as<8>(recs, n, dual, dst, dst_stride, s);
  else if (width <= 16) launch_readout_vectors_as<16>(recs, n, dual, dst, dst_stride, s);
  else if (width <= 32) launch_readout_vectors_as<32>(recs, n, dual, dst, dst_stride, s);
  else launch_readout_vectors_as<64>(recs, n, dual, dst, dst_stride, s);
}
template <int G, int CH>
static void launch_readout_beliefs_as(const ReadoutRec* recs, const DecodeLink* links, const double* dual, const double* cdata, double* dst,
                                      int64_t dst_stride, int64_t first, int64_t count, int tab32, hipStream_t s) {
  constexpr int GPB = 256 / G;
  hipLaunchKernelGGL((readout_beliefs_kernel<G, CH>), dim3((unsigned)((count + GPB - 1) / GPB)), dim3(256), 0, s, recs, links, dual, cdata, dst,
                     dst_stride, first, count, tab32);
}
void launch_readout_beliefs(const ReadoutRec* recs, const DecodeLink* links, const double* dual, const double* cdata, double* dst,
                            int64_t dst_stride, int64_t first, int64_t count, int width, int tab32, hipStream_t s) {
  if (count <= 0) return;
  if (width <= 4) launch_readout_beliefs_as<4, 1>(recs, links, dual, cdata, dst, dst_stride, first, count, tab32, s);
  else if (width <= 8) launch_readout_beliefs_as<8, 1>(recs, links, dual, cdata, dst, dst_stride, first, count, tab32, s);
  else if (width <= 16) launch_readout_beliefs_as<16, 1>(recs, links, dual, cdata, dst, dst_stride, first, count, tab32, s);
  else if (width <= READOUT_GROUP_MAX) launch_readout_beliefs_as<32, 1>(recs, links, dual, cdata, dst, dst_stride, first, count, tab32, s);
  else if (width <= 64) launch_readout_beliefs_as<64, 1>(recs, links, dual, cdata, dst, dst_stride, first, count, tab32, s);
  else launch_readout_beliefs_as<64, READOUT_CHUNK / 64>(recs, links, dual, cdata, dst, dst_stride, first, count, tab32, s);
}

// ---- moving label windows (prepared.cpp, lpmp_move_windows) ---------------------------------------------------------
// The window of a listed unary moves by delta labels: new label x is old label x + delta, labels that enter the window copy the
// nearest old end value — v'[x] = v[g(x)], g(x) = clamp(x + delta, 0, d0 - 1) — for theta and for the unary's message vector in every
// adjacent pairwise factor.  One wave per listed unary; a vector of up to MOVE_MAX_LABELS labels is held in registers, lane l the
// labels l, l + 64, ...  The gather is IN PLACE: with delta < 0 label x reads an entry that label x + delta — another lane, or the
// same lane's earlier register — overwrites, so every load of a vector has returned (the explicit wait) before its first store is
// issued.  No LDS, no atomics, plain 8-byte loads and stores, 64-bit offsets.  A device delta is saturated where it is read.
__device__ __forceinline__ int move_delta(const int32_t* __restrict__ delta, int row) {
  return row < 0 ? 0 : min(max(delta[row], -MOVE_DELTA_MAX), MOVE_DELTA_MAX);
}
__global__ void __launch_bounds__(256)
move_windows_kernel(const MoveRec* __restrict__ recs, const MoveLink* __restrict__ links, int64_t n, const int32_t* __restrict__ delta,
                    double* dual, double* __restrict__ lb, const double* __restrict__ cost_old, const double* __restrict__ cost_new,
                    int64_t cost_stride) {
  constexpr int PER = MOVE_MAX_LABELS / 64;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * 4 + wave;
  if (k >= n) return;
  const MoveRec r = recs[k];
  const int d = r.d0, dl = move_delta(delta, r.row);
  int g[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) g[j] = min(max(lane + 64 * j + dl, 0), d - 1);
  double v[PER];
  {
    double* th = dual + r.dual_off;
#pragma unroll
    for (int j = 0; j < PER; ++j) if (lane + 64 * j < d) v[j] = th[g[j]];
    if (cost_old) {   // (wave-uniform) the new unary costs: the inner difference first, skipped where the two entries compare equal
      const double* co = cost_old + (int64_t)r.row * cost_stride;
      const double* cn = cost_new + (int64_t)r.row * cost_stride;
#pragma unroll
      for (int j = 0; j < PER; ++j)
        if (lane + 64 * j < d) {
          const double a = cn[lane + 64 * j], b = co[g[j]];
          if (!(a == b)) v[j] = v[j] + (a - b);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every load of the vector has returned: no store overtakes one
#pragma unroll
    for (int j = 0; j < PER; ++j) if (lane + 64 * j < d) th[lane + 64 * j] = v[j];
  }
  for (int i = 0; i < r.n_links; ++i) {
    double* m = dual + links[r.link_begin + i].vec_off;
#pragma unroll
    for (int j = 0; j < PER; ++j) if (lane + 64 * j < d) v[j] = m[g[j]];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < PER; ++j) if (lane + 64 * j < d) m[lane + 64 * j] = v[j];
  }
  if (lane == 0) lb[r.factor] = __longlong_as_double(-1LL);   // stale, as set_vectors_kernel marks it
}
// the shifts of the DIFF_SHIFT factors next to the listed unaries: cost(a, b) = scale * D[clip(a - b + s)] stays the same function of
// the ABSOLUTE labels exactly when s' = s + delta_left - delta_right.  One thread per factor; the constants are written (both
// places, as set_constants_kernel writes a DIFF_SHIFT row) only when the two deltas differ, the bound is stale either way — the
// factor's message vectors have moved
__global__ void __launch_bounds__(256)
move_shifts_kernel(const MoveShiftRec* __restrict__ recs, int64_t n, const int32_t* __restrict__ delta, double* __restrict__ cdata,
                   double* __restrict__ lb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const MoveShiftRec r = recs[i];
  const int dl = move_delta(delta, r.left_row), dr = move_delta(delta, r.right_row);
  if (dl != dr) {
    const int s = diff_shift_int(cdata[r.cell]) + dl - dr;      // |s| <= 2^30 + 2^21
    const double v = (double)min(max(s, -(1 << 30)), 1 << 30);
    cdata[r.cell] = v;
    cdata[r.packed] = v;
  }
  lb[r.factor] = __longlong_as_double(-1LL);
}
void launch_move_windows(const MoveRec* recs, const MoveLink* links, int64_t n, const int32_t* delta, double* dual, double* lb,
                         const double* cost_old, const double* cost_new, int64_t cost_stride, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(move_windows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, recs, links, n, delta, dual, lb, cost_old, cost_new, cost_stride);
}
void launch_move_shifts(const MoveShiftRec* recs, int64_t n, const int32_t* delta, double* cdata, double* lb, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(move_shifts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, recs, n, delta, cdata, lb);
}

// ---- primal state on the device (prepared.cpp: lpmp_readout_set_labels, lpmp_move_windows_carry; engine.cpp: lpmp_lower_bound_dev,
// lpmp_evaluate_primal_dev) ------------------------------------------------------------------------------------
// Plain launches on the engine's stream: no LDS, no atomics, plain vector stores, 64-bit indexing of primal[2 * f].
// labels in: the input twin of readout_labels_kernel.  One thread per listed factor; src[row] is its label, the dimension (or any
// value outside [0, d0 - 1]: no bit pattern reaches the primal array unchecked) means unset.  A read-out with a factor listed
// twice never gets here (prepared.cpp), so every slot has one writer
__global__ void __launch_bounds__(256)
set_labels_kernel(const ReadoutRec* __restrict__ recs, int64_t n, const int32_t* __restrict__ src, int32_t* __restrict__ primal) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const ReadoutRec r = recs[i];
  const int32_t x = src[r.row];
  primal[2 * (int64_t)r.factor] = (x >= 0 && x < r.d0) ? x : r.d0;
}
// labels carried through a window move: new label x is old label x + delta, so the label that named old x names x - delta now,
// clamped into the window (the nearest absolute label that stayed).  One thread per listed unary; the delta is saturated as
// move_windows_kernel saturates it; an unset slot (the dimension, or whatever else is no label) is left as it is
__global__ void __launch_bounds__(256)
carry_labels_kernel(const MoveRec* __restrict__ recs, int64_t n, const int32_t* __restrict__ delta, int32_t* __restrict__ primal) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const MoveRec r = recs[i];
  const int32_t x = primal[2 * (int64_t)r.factor];
  if (x < 0 || x >= r.d0) return;
  primal[2 * (int64_t)r.factor] = min(max(x - move_delta(delta, r.row), 0), r.d0 - 1);
}
// factor_lb_list_kernel with the length of the list read from the device counter lb_collect_stale_kernel left: a fixed grid, a
// wave per entry, grid-stride (the host never learns the count)
__global__ void __launch_bounds__(256)
factor_lb_list_dev_kernel(const LbRec* __restrict__ recs, const double* __restrict__ dual, const double* __restrict__ cdata,
                          double* __restrict__ out, const int32_t* __restrict__ list, const unsigned long long* __restrict__ counter, int tab32) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t count = (int64_t)*counter, stride = (int64_t)gridDim.x * 4;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < count; i += stride) {
    const int32_t f = list[i];
    const double lb = factor_lb(recs[f], dual, cdata, tab32, lane);
    if (lane == 0) out[f] = lb;
  }
}
// the second stage of the two-stage sum, as the host adds it: the model constant plus the partial sums of sum_stage_kernel in
// ascending order, one thread, one IEEE add each.  bad != nullptr: the consistency flag of primal_check_kernel; set: +inf
__global__ void __launch_bounds__(64)
sum_final_kernel(const double* __restrict__ part, int64_t n_part, double constant, const int* __restrict__ bad, double* __restrict__ dst) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double s = constant;
  for (int64_t i = 0; i < n_part; ++i) s += part[i];
  if (bad && *bad != 0) s = LPMP_INF;
  *dst = s;
}
void launch_set_labels(const ReadoutRec* recs, int64_t n, const int32_t* src, int32_t* primal, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(set_labels_kernel, blocks256(n), dim3(256), 0, s, recs, n, src, primal);
}
void launch_carry_labels(const MoveRec* recs, int64_t n, const int32_t* delta, int32_t* primal, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(carry_labels_kernel, blocks256(n), dim3(256), 0, s, recs, n, delta, primal);
}
void launch_factor_lb_list_dev(const LbRec* recs, const double* dual, const double* cdata, double* out, const int32_t* list,
                               const unsigned long long* counter, int64_t max_count, int tab32, hipStream_t s) {
  if (max_count <= 0) return;
  int64_t blocks = (max_count + 3) / 4;
  if (blocks > LB_LIST_DEV_BLOCKS) blocks = LB_LIST_DEV_BLOCKS;
  hipLaunchKernelGGL(factor_lb_list_dev_kernel, dim3((unsigned)blocks), dim3(256), 0, s, recs, dual, cdata, out, list, counter, tab32);
}
void launch_sum_final(const double* part, int64_t n_part, double constant, const int* bad, double* dst, hipStream_t s) {
  hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(64), 0, s, part, n_part, constant, bad, dst);
}

}  // namespace lpmp
