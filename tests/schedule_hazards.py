"""Host-side hazard checker for planned schedules and chain plans (helpers; the tests are in test_schedule_hazards_host.py).

The device tests compare values; a wrong *schedule* is a race that an idle GPU usually wins.  This module decides on the host,
deterministically, whether every pair of conflicting updates of a planned sweep is ordered by something the executor enforces.

Ground truth (not from plan.cpp)
--------------------------------
`footprint()` gives what one update — factor f, its omega row, its receive-mask row — reads and writes, derived from what
oracle/lpmp_oracle.c dereferences (update_factor, message_delta, apply_delta, repam_left / repam_right) and from the message
lists of `Oracle.msg_lists()`.  Vectors are numbered 2 * factor + side: a vector factor (and a labeling-list / min-norm peer) is
the one vector 2 f, a pairwise factor has the halves 2 p (side 0) and 2 p + 1 (side 1).

  * an update with an active message (or of a COMPUTE_PRIMAL type) reads all of its own dual;
  * f on the LEFT of the message (role 0, peer g on the right):
      receive: message_delta reads ALL of g (both halves and the table), repam_right writes g's half `side` (all of a vector
               peer), repam_left writes f;
      send:    delta from f's snapshot; repam_right reads and writes g's half `side`, repam_left writes f;
  * f on the RIGHT (role 1, peer g a vector): receive reads g, writes g and f's half `side`; send writes g and f's half `side`.
  * a send is active when its weight is non-zero; with batch sends (effective_send_weights) that is the same set.
  * NOT covered: the adaptive send rule (message_improvement reads all of the peer for every send).  The oracle cannot tell the
    wider footprint from this one on the sweeps tried (no linear extension differed with either), so it is left out, not guessed.

Two updates conflict when one writes what the other reads or writes.  test_footprints_are_sufficient_for_the_oracle pins this
relation against the oracle (random linear extensions of the conflict DAG reproduce the sequential sweep bit for bit).

Rounding passes: `Oracle` has no iterator-range rounding pass, and propagate_primal_through_messages recurses through the graph,
so primal slots have no bounded footprint here.  What is taken from the oracle's rounding functions and from engine.cpp
ensure_primal's stated rule is: a record of a COMPUTE_PRIMAL type exists even without an active message and reads its own dual
(maximize_potential_and_compute_primal), and a PAIRWISE factor that rounds itself touches (reads and writes) all its unaries,
active or not (`Footprint.primal`).  These are checked in one direction only: the planner must order at least these accesses.
The last rule holds in primal passes only, and engine.cpp run_schedule (:750-753) never runs a primal pass in the chain form when
the model has such factors (d_pw_unary set) or a chain of an op-by-op class: the plain form is checked with it, the chain form
without it.  chain_plan.cpp `replay` accordingly never visits those accesses; nothing has to be added there.

Device-only state: tracked lower bounds (from kernels.hip, not from the oracle)
--------------------------------------------------------------------------------
Every record of f stores lb[f]; an op stores lb[peer] (st_lb in kernels.hip) unless it is a send whose vector goes to the mailbox
("a vector that goes to the mailbox has a reader later in this launch, which sets the peer's tracked bound itself"), or a receive
whose result is forwarded in a register to a send of the same record (Op::pad of the send = index of the receive + 1: the send
stores the slot instead).  Slots are write-only inside a sweep; two records writing one slot are a write-write pair.

The executor ("What orders what on the device")
-----------------------------------------------------------
plain:  engine.cpp issue_launches: the launches complete in list order; records of one launch run concurrently.
chain:  engine.cpp run_schedule: Schedule::plain_launches in order, then every chain as ONE launch in the order of
        Schedule::chains.  Level loop: its launches in order, one workgroup.  Ticket chain: a ticket (block tk_block of launch
        tk_launch) starts when the tickets of its dep list have completed; tickets are handed out in increasing order to a
        bounded number of resident workgroups, so a dep on a later ticket is a deadlock.
granule: a receive with OP_MAILBOX takes its vector from a mailbox row instead of the dual array.  Program order of a record in
        the mailbox form of the packed bodies (kernels.hip dense_pk_body): S — the dep flags are seen and every dual the record
        reads from memory is requested; K — the rows are taken and all those loads are awaited, BEFORE the record's first store;
        P — the sends: mailbox_put of a vector, then its store to the dual array; E — the late lb[] stores, completion, flag.
        The value a send puts depends on the record's dual after all its receives, so everything up to K of the producer — its
        reads in the receive phase, of its own dual, of the targets of its first MAILBOX_SENDS sends (the ones requested up front),
        and whatever had completed before the producer started — is before what the consumer does after ITS K, i.e. before the
        consumer's stores.  A granule does NOT order the consumer's own loads from memory (requested at S, before the take) and does
        NOT make the producer's stores to the dual array or to lb[] visible (they are issued after the put).  `Reach` holds exactly
        this graph: S -> K -> P -> E per ticket, E(d) -> S(t) per dep, P(a) -> K(b) per hand-over.  A pair is ordered when:
        read-after-write: the vector comes from the row and no other op of the consumer reads it from memory; else E(a) -> S(b);
        write-after-write (duals and lb[]): E(a) -> K(b);  write-after-read: P(a) -> K(b) if the read is one of the early reads
        named above, else E(a) -> K(b).  chain_plan.cpp's comment on the hand-over ("w's own reads of g precede that send in w's
        program order") states the write-after-read part of this contract; the kernel agrees with it.

Out of scope: the joined-pass launches (engine.cpp rotation_chain / order.cpp joined_pass_tables; their records are templates
expanded over passes — `conflict_edges` and `Reach` are written to be reused there), the multi-GPU hosts, and whether the kernels
implement flags and granules correctly (the GPU parity tests).
"""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
from collections import defaultdict

import numpy as np

from lp_mp_amd import model as M
from oracle.binding import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lp_mp_amd", "csrc")

CHAIN_LAUNCH_LABEL_OPS, CHAIN_LAUNCH_LABEL_PAIRED, CHAIN_LAUNCH_MAILBOX = 1, 2, 1 << 30
UPD_PRIMAL = 1 << 17
KC_GENERIC, KC_DENSE_4, KC_POTTS_V32, KC_SMALL, KC_SHARED_4, KC_SHARED_32 = 0, 1, 16, 18, 23, 26


def kc_is_packed(c):
    return KC_DENSE_4 <= c <= KC_POTTS_V32


def kc_is_shared(c):
    return KC_SHARED_4 <= c <= KC_SHARED_32


# ---------------------------------------------------------------------------------------------------------------------------
# model view and footprints (oracle side)

def _sends_to_left(s):
    return s in (M.SCHED_RIGHT, M.SCHED_FULL, M.SCHED_ONLY_SEND)


def _sends_to_right(s):
    return s in (M.SCHED_LEFT, M.SCHED_FULL, M.SCHED_ONLY_SEND)


def _recv_from_left(s):
    return s in (M.SCHED_RIGHT, M.SCHED_FULL)


def _recv_from_right(s):
    return s in (M.SCHED_LEFT, M.SCHED_FULL)


class ModelInfo:
    """per-factor message lists in the oracle's order, with what each entry may do"""

    def __init__(self, model):
        self.model = model
        self.oracle_model = model.expand_diff().expand_shared() if (model.has_shared or model.has_diff) else model
        o = Oracle(self.oracle_model)
        off, ent = o.msg_lists()
        self.fm_off = off.tolist()
        msg = (ent >> 1).astype(np.int64)
        role = (ent & 1).astype(np.int64)
        mt = model.m_type[msg]
        sched = [model.mtypes[t].schedule for t in mt]
        self.fm_msg = msg.tolist()
        self.fm_role = role.tolist()
        self.fm_mtype = [int(t) for t in mt]
        self.fm_kind = [model.mtypes[t].kind for t in mt]
        self.fm_side = [model.mtypes[t].param if model.mtypes[t].kind == M.M_UNARY_PAIRWISE else 0 for t in mt]
        self.fm_adj = np.where(role == 0, model.m_right[msg], model.m_left[msg]).tolist()
        self.fm_sends = [(_sends_to_right(s) if r == 0 else _sends_to_left(s)) for s, r in zip(sched, self.fm_role)]
        self.fm_recvs = [(_recv_from_right(s) if r == 0 else _recv_from_left(s)) for s, r in zip(sched, self.fm_role)]
        self.pairwise = (model.f_kind != M.F_VECTOR).tolist()
        cp = model.ftype_computes_primal
        self.primal_type = [bool(cp is not None and len(cp) and cp[t]) for t in model.f_type]
        self.any_batch = any(t.flags & (M.MF_BATCH_TO_RIGHT | M.MF_BATCH_TO_LEFT) for t in model.mtypes)
        self.nf = model.n_factors

    def n_sends(self, f):
        return sum(self.fm_sends[self.fm_off[f]:self.fm_off[f + 1]])

    def n_recvs(self, f):
        return sum(self.fm_recvs[self.fm_off[f]:self.fm_off[f + 1]])

    def vectors_of(self, f):
        return (2 * f, 2 * f + 1) if self.pairwise[f] else (2 * f,)

    def effective_send_weights(self, f, om):
        """CallSendMessages' batch rule as oracle/lpmp_oracle.c effective_send_weights states it"""
        if not self.any_batch:
            return list(om)
        w, k, j, e = [], 0, self.fm_off[f], self.fm_off[f + 1]
        while j < e:
            j2 = j
            while j2 < e and self.fm_mtype[j2] == self.fm_mtype[j] and self.fm_role[j2] == self.fm_role[j]:
                j2 += 1
            if self.fm_sends[j]:
                n = j2 - j
                fl = self.model.mtypes[self.fm_mtype[j]].flags
                batch = bool(fl & (M.MF_BATCH_TO_RIGHT if self.fm_role[j] == 0 else M.MF_BATCH_TO_LEFT))
                row = [float(x) for x in om[k:k + n]]
                if batch:
                    n_active, total = 0, 0.0
                    for x in row:
                        n_active += x > 0.0
                        total += x
                    if n_active > 1:
                        each = total / float(n_active)
                        w += [each if x > 0.0 else 0.0 for x in row]
                    else:
                        w += [x if x > 0.0 else 0.0 for x in row]
                else:
                    w += row
                k += n
            j = j2
        return w


class Footprint:
    __slots__ = ("reads", "writes", "primal", "recv_ops", "send_ops", "is_record")

    def __init__(self):
        self.reads, self.writes = set(), set()
        self.primal = set()                        # primal passes only: the vectors a pairwise factor that rounds itself touches
        self.recv_ops, self.send_ops = [], []      # (peer, side, role, kind[, omega]) in message-list order
        self.is_record = False

    def access(self, primal=True):
        return (self.reads | self.primal, self.writes | self.primal) if primal and self.primal else (self.reads, self.writes)


def footprint(mi, f, om, mk):
    """what one update reads and writes (module docstring); om: the weight row as given (not the effective weights)"""
    fp = Footprint()
    w = mi.effective_send_weights(f, om)
    ks = kr = 0
    own = mi.vectors_of(f)
    for j in range(mi.fm_off[f], mi.fm_off[f + 1]):
        g, role, kind, side = mi.fm_adj[j], mi.fm_role[j], mi.fm_kind[j], mi.fm_side[j]
        recv = send = False
        if mi.fm_recvs[j]:
            recv = bool(mk[kr]); kr += 1
        if mi.fm_sends[j]:
            omega = float(w[ks]); send = omega != 0.0; ks += 1
        if not (recv or send):
            continue
        if role == 0:
            gv = 2 * g + side if kind == M.M_UNARY_PAIRWISE else 2 * g
            if recv:
                fp.reads.update(mi.vectors_of(g)); fp.writes.add(gv)
            if send:
                fp.reads.add(gv); fp.writes.add(gv)
            fp.writes.add(2 * f)
        else:
            fv = 2 * f + side if kind == M.M_UNARY_PAIRWISE else 2 * f
            fp.reads.add(2 * g); fp.writes.add(2 * g); fp.writes.add(fv)
        if recv:
            fp.recv_ops.append((g, side, role, kind))
        if send:
            fp.send_ops.append((g, side, role, kind, omega))
    fp.is_record = bool(fp.recv_ops or fp.send_ops or mi.primal_type[f])
    if fp.is_record:
        fp.reads.update(own)
    if mi.primal_type[f] and mi.pairwise[f]:
        # engine.cpp ensure_primal: a pairwise factor that rounds itself reads and writes the labels of all its unaries
        for j in range(mi.fm_off[f], mi.fm_off[f + 1]):
            fp.primal.add(2 * mi.fm_adj[j])
        fp.primal.update(own)
    return fp


def conflict_edges(accesses):
    """accesses: per node (reads, writes).  The generating pairs (a, b, vector, kind), a < b, of the conflict relation: last
    writer -> reader (RAW), last writer -> writer (WAW), readers since the last write -> writer (WAR).  Every other conflicting
    pair follows from these by transitivity."""
    last_w, readers, out = {}, defaultdict(list), []
    for b, (R, W) in enumerate(accesses):
        for v in R:
            a = last_w.get(v)
            if a is not None and a != b:
                out.append((a, b, v, "RAW"))
        for v in W:
            a = last_w.get(v)
            if a is not None and a != b and v not in R:
                out.append((a, b, v, "WAW"))
            for a in readers.get(v, ()):
                if a != b:
                    out.append((a, b, v, "WAR"))
        for v in W:
            last_w[v] = b; readers[v] = []
        for v in R:
            if v not in W:
                readers[v].append(b)
    return out


class Sequence:
    """the update list of one or several sweeps: factor, weight row, mask row per update, and the footprints"""

    def __init__(self, mi, factors, om_off, om, mk_off, mk):
        self.mi = mi
        self.factor = [int(f) for f in factors]
        self.om = [np.asarray(om[om_off[i]:om_off[i + 1]], np.float64) for i in range(len(self.factor))]
        self.mk = [np.asarray(mk[mk_off[i]:mk_off[i + 1]], np.uint8) for i in range(len(self.factor))]
        self.fp = [footprint(mi, f, o, m) for f, o, m in zip(self.factor, self.om, self.mk)]
        self._edges = {}

    def __len__(self):
        return len(self.factor)

    def edges(self, primal=True):
        """the generating pairs of the conflict relation; primal: with the accesses of primal passes"""
        if primal not in self._edges:
            self._edges[primal] = conflict_edges([fp.access(primal) for fp in self.fp])
        return self._edges[primal]

    def rows(self, perm):
        """(factors, om_off, om, mk_off, mk) of the updates in the order perm"""
        f = np.array([self.factor[i] for i in perm], np.int32)
        oms, mks = [self.om[i] for i in perm], [self.mk[i] for i in perm]
        om_off = np.concatenate([[0], np.cumsum([len(x) for x in oms])]).astype(np.int64)
        mk_off = np.concatenate([[0], np.cumsum([len(x) for x in mks])]).astype(np.int64)
        om = np.concatenate(oms) if oms and om_off[-1] else np.zeros(0)
        mk = np.concatenate(mks) if mks and mk_off[-1] else np.zeros(0, np.uint8)
        return f, om_off, om.astype(np.float64), mk_off, mk.astype(np.uint8)


def linear_extension(n, edges, rng, adversarial):
    """a linear extension of the DAG; adversarial: always the LATEST ready node, else a random ready one"""
    import heapq
    succ, indeg = defaultdict(list), [0] * n
    for a, b in set((a, b) for a, b, _, _ in edges):
        succ[a].append(b); indeg[b] += 1
    ready = [i for i in range(n) if indeg[i] == 0]
    out = []
    if adversarial:
        heap = [-i for i in ready]
        heapq.heapify(heap)
        while heap:
            a = -heapq.heappop(heap); out.append(a)
            for b in succ[a]:
                indeg[b] -= 1
                if indeg[b] == 0:
                    heapq.heappush(heap, -b)
    else:
        while ready:
            k = int(rng.integers(len(ready)))
            ready[k], ready[-1] = ready[-1], ready[k]
            a = ready.pop(); out.append(a)
            for b in succ[a]:
                indeg[b] -= 1
                if indeg[b] == 0:
                    ready.append(b)
    assert len(out) == n
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the probe library (tests/cpp/schedule_probe.cpp + the planner sources, g++ alone)

SETTING_DEFAULTS = dict(chain_min=9, chain_all=0, no_level_loop=0, no_blocked_passes=0, band_min_bytes=64 << 20, band_min_set=0,
                        band_bytes=16 << 20, heavy_bytes=256 << 20, no_mailbox=0, verbose=0)


def build_probe(out_dir):
    # (tools/sanitize_host.sh: another compiler and sanitizer flags for the probe and the planner sources it is built with)
    gxx = os.environ.get("LPMP_PROBE_CXX") or shutil.which("g++")
    if gxx is None:
        raise RuntimeError("g++ not found")
    so = os.path.join(str(out_dir), "libschedule_probe.so")
    cmd = [gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"] + os.environ.get("LPMP_PROBE_CXXFLAGS", "").split() + ["-I", CSRC, "-o", so,
           os.path.join(ROOT, "tests", "cpp", "schedule_probe.cpp")] + [os.path.join(CSRC, f) for f in ("plan.cpp", "chain_plan.cpp", "order.cpp")] + ["-lpthread"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError(out.stdout[-3000:] + out.stderr[-3000:])
    L = C.CDLL(so)
    L.probe_create.restype = C.c_void_p
    L.probe_create.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_char_p, C.c_int]
    L.probe_destroy.argtypes = [C.c_void_p]
    L.probe_error.restype = C.c_char_p
    L.probe_error.argtypes = [C.c_void_p]
    L.probe_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_int]
    L.probe_get.restype = C.c_int64
    L.probe_get.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
    L.probe_setting_name.restype = C.c_char_p
    L.probe_setting_name.argtypes = [C.c_int]
    return L


def probe_setting_names(L):
    return [L.probe_setting_name(i).decode() for i in range(L.probe_n_settings())]


def chain_settings_fields():
    """the members of struct ChainSettings in plan.hpp: every declaration that ends in `;`, whatever its type"""
    src = open(os.path.join(CSRC, "plan.hpp")).read()
    body = re.search(r"struct ChainSettings \{(.*?)\n\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = []
    for decl in body.split(";"):
        decl = decl.split("=")[0].strip()
        if decl:
            names.append(re.findall(r"\w+", decl)[-1])
    return names


_REC = ("rec_launch", "rec_level", "rec_class", "rec_factor", "rec_n_recv", "rec_n_send", "rec_op_begin", "rec_kind_flags",
        "rec_dual_off", "rec_const_off", "pk_rec_dual_off", "pk_rec_const_off")
_OP = ("op_peer", "op_side", "op_role", "op_code", "op_pad", "op_omega_bits", "op_mailbox_row",
       "op_peer_dual", "op_peer_const", "pk_op_peer_dual", "pk_op_peer_const")
_LAUNCH = ("launch_class", "launch_begin", "launch_end", "launch_level", "launch_stride", "launch_n_recv", "launch_bytes", "launch_n_sh", "plain_launches", "n_levels")
_CHAIN = ("chain_class", "chain_block_records", "chain_level_loop", "chain_banded", "chain_valid", "chain_mailbox_rows", "chain_mailbox_width", "mailbox_sends")
_PER_CHAIN = ("cl_rec_begin", "cl_count", "cl_ticket0", "cl_flags", "tk_launch", "tk_block", "dep_off", "dep")
# read-only words of the records, the ops and their packet copies: where a factor lies in the dual / const arrays, in elements
# (Python ints via .tolist(); pk_*: NO_PACKET where the launch has no packets) — tests/test_far_offsets_host.py
NO_PACKET = -(1 << 63)
_SEQ = ("seg_n", "seq_factor", "seq_om_off", "seq_mk_off", "seq_mk", "seq_om_bits")


class Probe:
    def __init__(self, L, model, force_generic=False, mailbox_budget_bytes=-1):
        self.L, self.model = L, model
        cs = model.c_struct()
        err = C.create_string_buffer(512)
        self.h = L.probe_create(C.addressof(cs), int(force_generic), int(mailbox_budget_bytes), err, 512)
        if not self.h:
            raise RuntimeError(err.value.decode())

    def __del__(self):
        if getattr(self, "h", None):
            self.L.probe_destroy(self.h); self.h = None

    def _get(self, name, chain=-1):
        n = self.L.probe_get(self.h, name.encode(), chain, None)
        if n < 0:
            raise KeyError(name)
        out = np.empty(max(n, 1), np.int64)
        self.L.probe_get(self.h, name.encode(), chain, out.ctypes.data)
        return out[:n]

    def plan(self, segments=None, fuse=False, settings=None, partition=None):
        """segments: list of (factors, om_off, om, mk_off, mk); partition: (rtype, inner_iterations) instead.
        Returns the schedule as a dict of arrays (chains: a list of dicts)."""
        names = probe_setting_names(self.L)
        st = dict(SETTING_DEFAULTS); st.update(settings or {})
        assert set(st) == set(names), (sorted(st), names)
        sv = np.array([int(st[k]) for k in names], np.int64)
        if partition is None:
            seg_n = np.array([len(s[0]) for s in segments], np.int64)
            cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(s[k], dt) for s in segments]) if segments else np.zeros(0, dt), dt)
            fa, oo, om, mo, mk = cat(0, np.int32), cat(1, np.int64), cat(2, np.float64), cat(3, np.int64), cat(4, np.uint8)
            rc = self.L.probe_plan(self.h, 0, 0, len(segments), seg_n.ctypes.data, fa.ctypes.data, oo.ctypes.data, om.ctypes.data, mo.ctypes.data,
                                   mk.ctypes.data, int(fuse), sv.ctypes.data, len(sv))
        else:
            rc = self.L.probe_plan(self.h, int(partition[0]), int(partition[1]), 0, None, None, None, None, None, None, int(fuse), sv.ctypes.data, len(sv))
        if rc != 0:
            raise RuntimeError(self.L.probe_error(self.h).decode())
        S = {k: self._get(k) for k in _REC + _OP + _LAUNCH + _CHAIN + _SEQ}
        S["chains"] = [{k: self._get(k, c) for k in _PER_CHAIN} for c in range(len(S["chain_class"]))]
        S["seq_om"] = S.pop("seq_om_bits").view(np.float64)
        return S


def sequence_of(mi, S):
    return Sequence(mi, S["seq_factor"], S["seq_om_off"], S["seq_om"], S["seq_mk_off"], S["seq_mk"])


def _lists(S):
    """the arrays of a schedule as Python lists (cached on the schedule: a mutated copy gets its own)"""
    if "_lists" not in S:
        X = {k: v.tolist() for k, v in S.items() if isinstance(v, np.ndarray)}
        X["chains"] = [{k: v.tolist() for k, v in c.items()} for c in S["chains"]]
        S["_lists"] = X
    return S["_lists"]


def copy_schedule(S):
    T = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in S.items() if k != "_lists"}
    T["chains"] = [{k: v.copy() for k, v in c.items()} for c in S["chains"]]
    return T


# ---------------------------------------------------------------------------------------------------------------------------
# the checker

class Violation:
    def __init__(self, kind, why, a=None, b=None, vector=None):
        self.kind, self.why, self.a, self.b, self.vector = kind, why, a, b, vector

    def __repr__(self):
        v = "" if self.vector is None else (" lb[%d]" % self.vector[1] if isinstance(self.vector, tuple) else " vector (factor %d, side %d)" % (self.vector >> 1, self.vector & 1))
        return "<%s: updates %s / %s%s: %s>" % (self.kind, self.a, self.b, v, self.why)


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def map_records(S, seq, out, fps=None):
    """rule (a): every update with a footprint is in exactly one record, whose ops are exactly the receives of its updates in
    sequence order, then their sends; folds only where the footprints allow.  Returns (rec_of_update, members_of_record)."""
    Sx = _lists(S)
    fps = seq.fp if fps is None else fps
    mi = seq.mi
    NR = len(Sx["rec_factor"])
    recs_of = defaultdict(list)
    order = sorted(range(NR), key=lambda i: (Sx["rec_launch"][i], i))
    for i in order:
        recs_of[Sx["rec_factor"][i]].append(i)
    upd_of = defaultdict(list)
    for u, f in enumerate(seq.factor):
        if fps[u].is_record:
            upd_of[f].append(u)
    rec_of = [-1] * len(seq)
    members = [[] for _ in range(NR)]
    for f in set(recs_of) | set(upd_of):
        us, k = upd_of.get(f, []), 0
        for i in recs_of.get(f, []):
            nr, ns, ob = Sx["rec_n_recv"][i], Sx["rec_n_send"][i], Sx["rec_op_begin"][i]
            if Sx["rec_launch"][i] < 0:
                out.append(Violation("mapping", "record %d of factor %d is in no launch" % (i, f)))
            run, r, s = [], 0, 0
            while k < len(us):
                u = us[k]; run.append(u); k += 1
                r += len(fps[u].recv_ops); s += len(fps[u].send_ops)
                if r >= nr and s >= ns:
                    break
            want = [(g, sd, ro, kd, _bits(1.0)) for u in run for (g, sd, ro, kd) in fps[u].recv_ops] + \
                   [(g, sd, ro, kd, _bits(w)) for u in run for (g, sd, ro, kd, w) in fps[u].send_ops]
            have = [(Sx["op_peer"][o], Sx["op_side"][o], Sx["op_role"][o], Sx["op_code"][o], Sx["op_omega_bits"][o]) for o in range(ob, ob + nr + ns)]
            if not run or r != nr or s != ns or want != have:
                out.append(Violation("mapping", "record %d of factor %d (%d receives, %d sends) does not hold the ops of updates %s" % (i, f, nr, ns, run), a=run[0] if run else None))
            if mi.primal_type[f] != bool(Sx["rec_kind_flags"][i] & UPD_PRIMAL):
                out.append(Violation("mapping", "record %d: UPD_PRIMAL does not match the factor type" % i))
            for u in run:
                rec_of[u] = i
            members[i] = run
            # a fold keeps program order only if no earlier member sends ...
            for x in run[:-1]:
                if fps[x].send_ops:
                    out.append(Violation("fold", "update %d sends and is followed by update %d in one record" % (x, run[-1]), a=x, b=run[-1]))
        if k < len(us):
            out.append(Violation("mapping", "updates %s of factor %d are in no record" % (us[k:], f), a=us[k]))
    # ... and no update between the first member and a later one conflicts with the later one
    for a, b, v, kind in (seq.edges() if fps is seq.fp else conflict_edges([fp.access() for fp in fps])):
        ra, rb = rec_of[a], rec_of[b]
        if ra < 0 or rb < 0 or ra == rb:
            continue
        if members[rb][0] < a:          # b was folded into a record that starts before a
            out.append(Violation("fold", "%s: update %d is folded into the record of update %d, across update %d" % (kind, b, members[rb][0], a), a=a, b=b, vector=v))
    return rec_of, members


class Reach:
    """happens-before inside one ticket chain (module docstring, granule).  Events: ("S", ticket) the dep flags seen, the loads from
    memory requested; ("K", record) its rows taken; ("P", record) its sends begin; ("E", ticket) complete, stores visible, flag
    published.  K and P are per RECORD: the records of a ticket are different waves that do not wait for each other.
    Edges: S(t) -> K(r) -> P(r) -> E(t) for the records r of t, E(d) -> S(t) per dep, P(a) -> K(b) per hand-over a -> b."""

    def __init__(self, dep_off, dep, rec_ticket=None, hand_overs=()):
        n = len(dep_off) - 1
        recs = defaultdict(list)
        for r, t in sorted((rec_ticket or {}).items()):
            recs[t].append(r)
        prod = defaultdict(list)
        for a, b in hand_overs:
            prod[b].append(a)
        self.nid, self.cl = {}, []
        for t in range(n):
            self._new(("S", t), [("E", int(d)) for d in dep[dep_off[t]:dep_off[t + 1]] if 0 <= d < t])
            for r in recs.get(t, ()):
                self._new(("K", r), [("S", t)] + [("P", w) for w in prod.get(r, ())])
                self._new(("P", r), [("K", r)])
            self._new(("E", t), [("S", t)] + [("P", r) for r in recs.get(t, ())])

    def _new(self, key, preds):
        c = 0
        for p in preds:
            i = self.nid.get(p)            # (a producer in a later ticket has no event yet: reported as a deadlock elsewhere)
            if i is not None:
                c |= self.cl[i] | (1 << i)
        self.nid[key] = len(self.cl)
        self.cl.append(c)

    def before(self, x, y, or_equal=False):
        if x == y:
            return or_equal
        i, j = self.nid.get(x), self.nid.get(y)
        return i is not None and j is not None and bool((self.cl[j] >> i) & 1)


class Executor:
    """what orders two records, per execution form (module docstring)"""

    def __init__(self, S, form, out):
        self.S, self.form = S, form
        Sx = _lists(S)
        NL = len(Sx["launch_class"])
        self.rec_launch = Sx["rec_launch"]
        self.unit = {}                     # launch -> (0, position) plain, (1, chain) chain
        self.chain_launch = {}             # launch -> index among its chain's launches
        self.ticket = {}                   # record -> ticket (ticket chains)
        self.reach, self.deps, self.takes = {}, {}, defaultdict(list)
        if form == "plain" or not len(Sx["chains"]):
            self.form = "plain"
            return
        begin_to_launch = {int(b): li for li, b in enumerate(Sx["launch_begin"]) if Sx["launch_end"][li] > b}
        for pos, li in enumerate(Sx["plain_launches"]):
            if li in self.unit:
                out.append(Violation("unit", "launch %d is issued twice" % li))
            self.unit[li] = (0, pos)
        for c, ch in enumerate(Sx["chains"]):
            gpb = Sx["chain_block_records"][c]
            level_loop = bool(Sx["chain_level_loop"][c])
            tk = {}
            for t, (k, b) in enumerate(zip(ch["tk_launch"], ch["tk_block"])):
                if (k, b) in tk:
                    out.append(Violation("ticket_map", "chain %d: block %d of launch %d has two tickets" % (c, b, k)))
                tk[(k, b)] = t
            for k, (rb, cnt) in enumerate(zip(ch["cl_rec_begin"], ch["cl_count"])):
                li = begin_to_launch.get(rb)
                if li is None or Sx["launch_end"][li] - Sx["launch_begin"][li] != cnt or Sx["launch_class"][li] != Sx["chain_class"][c]:
                    out.append(Violation("unit", "chain %d launch %d is no launch of the schedule" % (c, k)))
                    continue
                if li in self.unit:
                    out.append(Violation("unit", "launch %d is issued twice" % li))
                self.unit[li] = (1, c); self.chain_launch[li] = k
                if not level_loop:
                    for i in range(rb, rb + cnt):
                        t = tk.get((k, (i - rb) // gpb))
                        if t is None:
                            out.append(Violation("ticket_map", "chain %d: record %d has no ticket" % (c, i)))
                            t = -1
                        self.ticket[i] = t
            if not level_loop:
                off, dep = ch["dep_off"], ch["dep"]
                if len(off) != len(ch["tk_launch"]) + 1:
                    out.append(Violation("ticket_map", "chain %d: dep_off does not cover the tickets" % c))
                    off = off + [off[-1] if off else 0] * (len(ch["tk_launch"]) + 1 - len(off))
                for t in range(len(off) - 1):
                    for d in dep[off[t]:off[t + 1]]:
                        if d >= t or d < 0:
                            out.append(Violation("dep_forward", "chain %d: ticket %d waits for ticket %d (tickets are handed out in increasing order: a deadlock)" % (c, t, d)))
                self.deps[c] = (off, dep); self.reach[c] = None
        for li in range(NL):
            if Sx["launch_end"][li] > Sx["launch_begin"][li] and li not in self.unit:
                out.append(Violation("unit", "launch %d is never issued" % li))

    def add_granules(self, hand_overs, out):
        """hand_overs: (producer record, consumer record, index of the consumer's receive) of every mailbox row that is taken"""
        per = defaultdict(list)
        for ra, rb, k in hand_overs:
            c = self.unit[self.rec_launch[rb]][1]
            ta, tb = self.ticket.get(ra, -1), self.ticket.get(rb, -1)
            if not ta < tb:
                out.append(Violation("dep_forward", "chain %d: ticket %d polls a row that ticket %d writes (tickets are handed out in increasing order: a deadlock)" % (c, tb, ta)))
            per[c].append((ra, rb))
            self.takes[rb].append((k, ra))
        for c in self.deps:
            rt = {r: t for r, t in self.ticket.items() if self.unit[self.rec_launch[r]][1] == c}
            self.reach[c] = Reach(self.deps[c][0], self.deps[c][1], rt, per.get(c, ()))

    def ordered(self, ra, rb, kind="WAW", early_read=False, take_index=None):
        """the access of ra (a write, or the read of a WAR pair) happens before the access of rb: the read from memory of a RAW
        pair, else a write — by receive op take_index of rb, or (None) one that follows all its receives"""
        la, lb = self.rec_launch[ra], self.rec_launch[rb]
        if self.form == "plain":
            return la < lb, "launch %d is not before launch %d" % (la, lb)
        ua, ub = self.unit.get(la), self.unit.get(lb)
        if ua is None or ub is None:
            return False, "a launch that is never issued"
        if ua != ub:
            return ua < ub, "issue order: %s of launch %d is not before %s of launch %d" % (ua, la, ub, lb)
        if ua[0] == 0:
            return False, "both in plain launch %d" % la
        c = ua[1]
        if c not in self.reach:
            return self.chain_launch[la] < self.chain_launch[lb], "level loop: launch %d is not before launch %d" % (la, lb)
        ta, tb = self.ticket.get(ra, -1), self.ticket.get(rb, -1)
        if ta == tb:
            return False, "both in ticket %d" % ta
        R = self.reach[c]
        src = ("P", ra) if (kind == "WAR" and early_read) else ("E", ta)
        ok = R.before(src, ("S", tb))
        if not ok and kind != "RAW":
            # a store of rb follows the takes of its receives up to the one that stores (all of them for the sends and the own dual)
            ok = any((take_index is None or k <= take_index) and R.before(src, ("P", w), or_equal=True) for k, w in self.takes.get(rb, ()))
        return ok, "no dep / granule path from %s of ticket %d to the %s of ticket %d" % ("the early reads" if src[0] == "P" else "the end", ta, "start" if kind == "RAW" else "store", tb)

    def same_chain(self, ra, rb):
        ua, ub = self.unit.get(self.rec_launch[ra]), self.unit.get(self.rec_launch[rb])
        return self.form == "chain" and ua is not None and ua == ub and ua[0] == 1 and ua[1] in self.reach


def _op_vectors_of(S, mi, i):
    """per op of record i: (is_receive, vectors read from memory or mailbox, vectors written, the vector a mailbox moves)"""
    Sx = _lists(S)
    f, nr, ns, ob = Sx["rec_factor"][i], Sx["rec_n_recv"][i], Sx["rec_n_send"][i], Sx["rec_op_begin"][i]
    res = []
    for k in range(nr + ns):
        o = ob + k
        g, side, role, code = Sx["op_peer"][o], Sx["op_side"][o], Sx["op_role"][o], Sx["op_code"][o]
        if role == 0:
            gv = 2 * g + side if code == M.M_UNARY_PAIRWISE else 2 * g
            other = 2 * g + (1 - side) if (code == M.M_UNARY_PAIRWISE and mi.pairwise[g]) else None
            if k < nr:
                res.append((True, set(mi.vectors_of(g)), {gv, 2 * f}, other))
            else:
                res.append((False, {gv}, {gv, 2 * f}, gv))
        else:
            fv = 2 * f + side if code == M.M_UNARY_PAIRWISE else 2 * f
            res.append((k < nr, {2 * g}, {2 * g, fv}, None))
    return res


def lb_writes(S, i):
    """tracked-bound slots record i stores (module docstring; kernels.hip st_lb)"""
    Sx = _lists(S)
    f, nr, ns, ob = Sx["rec_factor"][i], Sx["rec_n_recv"][i], Sx["rec_n_send"][i], Sx["rec_op_begin"][i]
    w = {f}
    forwarded = {Sx["op_pad"][ob + nr + k] - 1 for k in range(ns) if Sx["op_pad"][ob + nr + k] > 0}
    for k in range(nr + ns):
        if k < nr and k in forwarded:
            continue
        if k >= nr and Sx["op_mailbox_row"][ob + k] >= 0:
            continue
        w.add(Sx["op_peer"][ob + k])
    return w


class Report(list):
    """the violations of one check ([] = sound), with what the check learnt on the way: members (the updates of every record) and
    stats (pairs checked, pairs ordered by a row itself, pairs between two units / two kernel classes)"""

    def __init__(self, members=None):
        super().__init__()
        self.members = members or []
        self.stats = defaultdict(int)


class _Check:
    """one run of the checker over one schedule in one execution form (the rules are those of the module docstring)"""

    def __init__(self, S, seq, fps, edges, executor, mapping):
        self.S, self.Sx, self.seq, self.mi, self.fps, self.edges = S, _lists(S), seq, seq.mi, fps, edges
        self.rec_of, self.members = mapping
        self.out = Report(self.members)
        self.ex = Executor(S, executor, self.out)
        self.first = [m[0] if m else -1 for m in self.members]
        self._ov = {}
        self.via_mailbox = defaultdict(dict)       # record -> vector -> (writer record, send index, receive index)

    def op_vectors(self, i):
        if i not in self._ov:
            self._ov[i] = _op_vectors_of(self.S, self.mi, i)
        return self._ov[i]

    def add(self, kind, why, a=None, b=None, vector=None):
        self.out.append(Violation(kind, why, a=a, b=b, vector=vector))

    def records(self):
        """per record: what its launch's kernel needs of it"""
        Sx, ex, first = self.Sx, self.ex, self.first
        for i in range(len(Sx["rec_factor"])):
            li = Sx["rec_launch"][i]
            cls = Sx["launch_class"][li]
            nr, ns, ob = Sx["rec_n_recv"][i], Sx["rec_n_send"][i], Sx["rec_op_begin"][i]
            label_flags = 0
            if ex.form == "chain" and ex.unit.get(li, (0, 0))[0] == 1:
                label_flags = Sx["chains"][ex.unit[li][1]]["cl_flags"][ex.chain_launch[li]]
            vec = [(Sx["op_peer"][ob + x], Sx["op_side"][ob + x]) for x in range(nr + ns)]
            if kc_is_packed(cls) or kc_is_shared(cls) or (label_flags & CHAIN_LAUNCH_LABEL_OPS):
                # receives are requested side by side, then the sends: no two of a kind into one vector
                for x in range(nr + ns):
                    for y in range(x + 1, nr + ns):
                        if (x < nr) == (y < nr) and vec[x] == vec[y]:
                            self.add("label_ops" if label_flags else "dup_vector", "record %d: ops %d and %d of one kind hit one vector in a class that runs them side by side" % (i, x, y), first[i], first[i])
            if label_flags & CHAIN_LAUNCH_LABEL_PAIRED:
                if nr != ns or any(vec[x] != vec[nr + x] for x in range(min(nr, ns))):
                    self.add("label_ops", "record %d: LABEL_PAIRED but send j does not go where receive j came from" % i, first[i], first[i])

    def chains(self):
        """every chain plan is valid, and the launches of a chain with a mailbox all carry CHAIN_LAUNCH_MAILBOX (kernels.hip picks
        the mailbox form of the body per launch) — and only those"""
        Sx = self.Sx
        for c, ch in enumerate(Sx["chains"]):
            if not Sx["chain_valid"][c]:
                self.add("unit", "chain %d is not valid" % c)
            want = Sx["chain_mailbox_rows"][c] > 0
            for k, fl in enumerate(ch["cl_flags"]):
                if bool(fl & CHAIN_LAUNCH_MAILBOX) != want:
                    self.add("mailbox_row", "chain %d with %d mailbox rows: launch %d %s CHAIN_LAUNCH_MAILBOX" % (c, Sx["chain_mailbox_rows"][c], k, "lacks" if want else "carries"))

    def mailbox_rows(self):
        """rule (d), the rows: inside the chain's mailbox, one writer per row among the first MAILBOX_SENDS sends, every polled row
        written, by a send into exactly the vector the receive wants"""
        Sx, ex, first = self.Sx, self.ex, self.first
        NR = len(Sx["rec_factor"])
        row_writer = {}

        def in_bounds(i, u, row):
            if u is None or u[0] != 1 or row >= Sx["chain_mailbox_rows"][u[1]]:
                self.add("mailbox_row", "record %d: row %d is outside the mailbox of its chain (%s rows)" % (i, row, Sx["chain_mailbox_rows"][u[1]] if u and u[0] == 1 else "no chain: 0"), first[i], first[i])
        for i in range(NR):
            nr, ns, ob = Sx["rec_n_recv"][i], Sx["rec_n_send"][i], Sx["rec_op_begin"][i]
            u = ex.unit.get(Sx["rec_launch"][i])
            for k in range(ns):
                row = Sx["op_mailbox_row"][ob + nr + k]
                if row < 0:
                    continue
                in_bounds(i, u, row)
                if (u, row) in row_writer:
                    self.add("mailbox_row", "row %d has two writers: records %d and %d" % (row, row_writer[(u, row)][0], i), first[row_writer[(u, row)][0]], first[i])
                if k >= Sx["mailbox_sends"][0]:
                    self.add("mailbox_row", "record %d: send %d writes a row but only the first %d sends can" % (i, k, Sx["mailbox_sends"][0]), first[i], first[i])
                row_writer[(u, row)] = (i, k, 2 * Sx["op_peer"][ob + nr + k] + Sx["op_side"][ob + nr + k])
        hand_overs = []
        for i in range(NR):
            nr, ob = Sx["rec_n_recv"][i], Sx["rec_op_begin"][i]
            u = ex.unit.get(Sx["rec_launch"][i])
            for k in range(nr):
                row = Sx["op_mailbox_row"][ob + k]
                if row < 0:
                    continue
                in_bounds(i, u, row)
                v = self.op_vectors(i)[k][3]
                w = row_writer.get((u, row))
                if w is None:
                    self.add("mailbox_writer", "record %d receive %d polls row %d that no send of its chain writes" % (i, k, row), first[i], first[i], v)
                elif v is None or w[2] != v:
                    self.add("mailbox_writer", "record %d receive %d polls row %d, which holds another vector (record %d send %d)" % (i, k, row, w[0], w[1]), first[w[0]], first[i], v)
                else:
                    self.via_mailbox[i][v] = (w[0], w[1], k)
                    hand_overs.append((w[0], i, k))
        ex.add_granules(hand_overs, self.out)

    def last_writers(self):
        """rule (d), the source: a vector taken from a row comes from the LAST writer of that vector before the update the receive
        belongs to (a folded record: the member that receives, not the first one)"""
        last_writer = {}
        for u in range(len(self.seq)):
            i = self.rec_of[u]
            if i >= 0 and self.via_mailbox.get(i):
                k0 = sum(len(self.fps[x].recv_ops) for x in self.members[i][:self.members[i].index(u)])
                for v, (w, _k, kr) in self.via_mailbox[i].items():
                    if not k0 <= kr < k0 + len(self.fps[u].recv_ops):
                        continue
                    lw = last_writer.get(v)
                    if lw is None or self.rec_of[lw] != w:
                        self.add("mailbox_writer", "record %d takes its vector from record %d, but its last writer before update %d is %s" % (i, w, u, "update %d" % lw if lw is not None else "nobody"), lw, u, v)
            for v in self.fps[u].writes:
                last_writer[v] = u

    def pairs(self):
        """rules (b), (c), (e), (f): every generating pair of the conflict relation is ordered by the executor, or (d) by a row"""
        Sx, ex, rec_of, members, stats = self.Sx, self.ex, self.rec_of, self.members, self.out.stats
        NR = len(Sx["rec_factor"])
        lbw = [lb_writes(self.S, i) for i in range(NR)]
        lb_acc = [(set(), {("lb", x) for x in lbw[rec_of[u]]} if rec_of[u] >= 0 and members[rec_of[u]][0] == u else set()) for u in range(len(self.seq))]
        seen = set()
        ms = Sx["mailbox_sends"][0]
        for a, b, v, kind in list(self.edges) + conflict_edges(lb_acc):
            ra, rb = rec_of[a], rec_of[b]
            if ra < 0 or rb < 0 or ra == rb or (ra, rb, v, kind) in seen:
                continue
            seen.add((ra, rb, v, kind))
            stats["pairs"] += 1
            la, lb = Sx["rec_launch"][ra], Sx["rec_launch"][rb]
            if Sx["launch_class"][la] != Sx["launch_class"][lb]:
                stats["cross_class_pairs"] += 1
            if ex.form == "chain":
                ua, ub = ex.unit.get(la), ex.unit.get(lb)
                if ua != ub and ua is not None and ub is not None and (ua[0] == 1 or ub[0] == 1):
                    stats["cross_unit_pairs"] += 1        # (two plain launches are ordered as in the plain form)
            if la == lb:
                self.add("same_launch", "%s: records %d and %d run concurrently in launch %d" % (kind, ra, rb, la), a, b, v)
                continue
            same_chain = ex.same_chain(ra, rb)
            if kind == "RAW" and same_chain and self.via_mailbox.get(rb, {}).get(v, (None,))[0] == ra:
                # taken from the row: ordered by the data itself, unless another op of the consumer reads the vector from memory
                ov = self.op_vectors(rb)
                nrb, obb = Sx["rec_n_recv"][rb], Sx["rec_op_begin"][rb]
                if not [k for k in range(len(ov)) if v in ov[k][1] and not (k < nrb and Sx["op_mailbox_row"][obb + k] >= 0 and ov[k][3] == v)]:
                    stats["pairs_ordered_by_the_row_itself"] += 1
                    continue
            early, take_index = False, None
            if kind == "WAR" and same_chain:
                # the producer's read precedes its mailbox_put: receive phase, own dual, or target of one of the first sends
                nra = Sx["rec_n_recv"][ra]
                er = set(self.mi.vectors_of(Sx["rec_factor"][ra]))
                for k, (is_recv, R, _W, _m) in enumerate(self.op_vectors(ra)):
                    if is_recv or k - nra < ms:
                        er |= R
                early = v in er
            if kind != "RAW" and same_chain:
                nrb, obb, fb = Sx["rec_n_recv"][rb], Sx["rec_op_begin"][rb], Sx["rec_factor"][rb]
                if isinstance(v, tuple):
                    js = [k for k in range(nrb) if Sx["op_peer"][obb + k] == v[1]]
                else:
                    js = [k for k, (is_recv, _R, W, _m) in enumerate(self.op_vectors(rb)) if is_recv and v in W and not (v == 2 * fb and Sx["op_role"][obb + k] == 0)]
                take_index = min(js) if js else None
            ok, why = ex.ordered(ra, rb, kind, early, take_index)
            if not ok:
                self.add({"plain": "launch_order"}.get(ex.form, "unordered"), "%s: %s" % (kind, why), a, b, v)


def check(S, seq, footprints=None, executor="chain", primal_in_chain=False, mapping=None):
    """violations of the planned schedule S (Probe.plan) against the update sequence seq, as a Report ([] = sound).
    executor: "plain" (launch by launch or graph replay) or "chain" (run_schedule with chain plans; the same as plain when the
    schedule has none).  footprints: other footprints than seq's own (seq is left alone).  The rule "a pairwise factor that rounds
    itself touches all its unaries" holds in primal passes only, and engine.cpp run_schedule never runs a primal pass of a model
    with such factors in the chain form (chain_ok = false when d_pw_unary is set): the chain form is checked without that rule
    unless primal_in_chain asks for it."""
    fps = seq.fp if footprints is None else footprints
    primal = executor == "plain" or not len(S["chains"]) or primal_in_chain
    edges = seq.edges(primal) if footprints is None else conflict_edges([fp.access(primal) for fp in fps])
    if mapping is None:
        pre = Report()
        mapping = map_records(S, seq, pre, fps)
    else:
        mapping, pre = mapping[:2], mapping[2]
    if any(v.kind == "mapping" for v in pre):
        pre.members = mapping[1]
        return pre                                        # the rest is meaningless without the mapping
    ck = _Check(S, seq, fps, edges, executor, mapping)
    ck.out.extend(pre)
    ck.records()
    if ck.ex.form == "chain":
        ck.chains()
        ck.mailbox_rows()
        ck.last_writers()
    ck.pairs()
    return ck.out


def check_all(S, seq):
    """both execution forms; the Report's stats are those of the chain form where the schedule has chains"""
    pre = Report()
    rec_of, members = map_records(S, seq, pre)
    out = check(S, seq, executor="plain", mapping=(rec_of, members, pre))
    if len(S["chains"]):
        chain = check(S, seq, executor="chain", mapping=(rec_of, members, []))
        chain.stats["cross_class_pairs"] = out.stats["cross_class_pairs"]
        chain[:0] = list(out)
        out = chain
    return out
