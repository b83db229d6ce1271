"""Models whose records sit AT the op-count caps of the packed sweep kernels and at the size limits of the device (kernels.hip:
dense_pk_body and its Potts, shared and updated-pairwise siblings stage a record and ALL its ops in a fixed LDS slab per lane group,
and the next lane group's slab starts right behind it).  No GPU and no pytest here: the caps restated, the builders, the case list,
what the planner must make of every case, and a census of the list.  tests/test_op_caps_host.py checks the list on the CPU,
tests/test_op_caps_gpu.py runs it on the device against the oracle.

Terms.  The OPS of a record are its active receives (mask != 0) plus its active sends (omega != 0) in one update.  In the two
anisotropic modes a variable receives from its earlier neighbours and sends to its later ones: degree ops; in the two uniform modes
every message is received AND sent: 2 x degree ops.  The CAP of a class is the number of ops its slab holds."""
import dataclasses
from typing import Callable, Optional

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

# ---- the caps, restated from lp_mp_amd/csrc/plan.hpp (tests/test_op_caps_host.py fails when the planner and these drift apart) ----
PK_MAX_OPS = 8                                      # PK_MAX_OPS: packet form up to here, indirect form above
INDIRECT_CAP = {4: 8, 8: 16, 16: 32, 32: 32}        # pk_indirect_cap: the Potts and shared classes, by padded width
DENSE_CAP = {4: 8, 8: 16, 16: 64, 32: 32}           # pk_dense_cap: the dense classes
PW_MAX_OPS = 6                                      # PW_MAX_OPS: updated pairwise factors
MAX_ACTIVE = 32767                                  # UpdRec::n_recv / n_send are int16_t (plan.cpp, bucket)
BIG_MAX_LABELS = 512                                # BIG_MAX_LABELS: the streaming class
SHARED_MAX_TABLES = 4                               # SHARED_MAX_TABLES: tables one launch of a shared class stages
SMALL_MAXD = 8                                      # SMALL_MAXD: the lane-per-factor class
MAILBOX_SENDS = 4                                   # MAILBOX_SENDS: a record with more sends keeps its completion flags

MODES = (M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2, M.REPAM_UNIFORM, M.REPAM_DAMPED_UNIFORM)
ANISO_MODES = (M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2)
DIRECTIONS = (M.FORWARD, M.BACKWARD)
WIDTHS = (4, 8, 16, 32)
VAR_LABELS = {4: 3, 8: 5, 16: 9, 32: 21}            # a label count of every run-time-dims class


def slot(w: int) -> int:
    """padded width of a label count up to 32"""
    return 4 if w <= 4 else 8 if w <= 8 else 16 if w <= 16 else 32


def class_cap(kclass: str) -> int:
    w = int(kclass[len(kclass.rstrip("0123456789")):])
    return DENSE_CAP[w] if kclass.startswith("dense") else PW_MAX_OPS if kclass.startswith("pairwise") else INDIRECT_CAP[w]


PACKED_CLASSES = (["dense%d" % w for w in WIDTHS] + ["potts%d" % w for w in WIDTHS] + ["dense_v%d" % w for w in WIDTHS] +
                  ["potts_v%d" % w for w in WIDTHS] + ["shared%d" % w for w in WIDTHS])
PAIRWISE_CLASSES = ["pairwise8", "pairwise16", "pairwise32"]      # (pairwise4 cannot occur: 4 + 4 duals fit the lane-per-factor class)


# ---- builders ----------------------------------------------------------------------------------------------------------------
def mrf(dims, ei, ej, pairwise: str, seed: int, compute_primal: bool = False) -> M.FlatModel:
    """variables 0 .. n-1 in index order with ``dims[v]`` labels, an edge per (ei[e], ej[e]) with ei < ej in lexicographic order;
    costs from default_rng(seed): unaries and dense tables uniform(0, 1) (never symmetric), Potts couplings uniform(0, 1) with a
    quarter of them -0.5, shared: SHARED_MAX_TABLES tables, one per edge at random, scale uniform(0.5, 2)"""
    dims = np.asarray(dims, np.int64); ei = np.asarray(ei, np.int64); ej = np.asarray(ej, np.int64)
    assert np.all(ei < ej) and ej.max() < dims.shape[0]
    o = np.lexsort((ej, ei)); ei, ej = ei[o], ej[o]
    n, E = dims.shape[0], ei.shape[0]
    rng = np.random.default_rng(seed)
    if np.all(dims == dims[0]):
        L = int(dims[0])
        un = rng.uniform(0, 1, (n, L))
        if pairwise == "dense":
            return S.mrf_model(n, L, ei, ej, un, tables=rng.uniform(0, 1, (E, L, L)), compute_primal=compute_primal)
        if pairwise == "potts":
            return S.mrf_model(n, L, ei, ej, un, potts=np.where(rng.random(E) < 0.25, -0.5, rng.uniform(0, 1, E)), compute_primal=compute_primal)
        assert pairwise == "shared"
        return S.mrf_model(n, L, ei, ej, un, compute_primal=compute_primal,
                           shared=(rng.uniform(0, 1, (SHARED_MAX_TABLES, L, L)), rng.integers(0, SHARED_MAX_TABLES, E), rng.uniform(0.5, 2, E)))
    assert pairwise == "dense", "rectangular tables are dense"
    b = M.ModelBuilder(2, S.mrf_mtypes(), [1, 0] if compute_primal else None)
    u = np.array([b.add_vector_factors(0, rng.uniform(0, 1, (1, int(d))))[0] for d in dims])
    p = np.array([b.add_dense_pairwise(1, rng.uniform(0, 1, (1, int(dims[i]), int(dims[j]))))[0] for i, j in zip(ei, ej)])
    b.add_interleaved_messages(np.tile(np.array([0, 1], np.int32), E), np.stack([u[ei], u[ej]], 1).reshape(-1), np.repeat(p, 2), return_ids=False)
    b.add_relations(np.stack([u[ei], p], 1).reshape(-1), np.stack([p, u[ej]], 1).reshape(-1))
    return b.finish()


def oracle_model(m: M.FlatModel) -> M.FlatModel:
    """what the oracle runs: SHARED factors expanded to dense tables (same factor order and dual layout; the oracle has no such kind)"""
    return m.expand_shared() if m.has_shared else m


def hub_side(L, pairwise, degrees, leaf_L=None, seed=1, compute_primal=False) -> M.FlatModel:
    """a bipartite model in colour-major order: side A the hubs, one per entry of ``degrees``, then side B the leaves, as many as the
    largest degree; hub k is joined to leaves k, k + 1, ... cyclically.  All hubs are one level: where they share a class, ONE
    launch with neighbouring slabs in one workgroup.  ``leaf_L``: another label count for the leaves (rectangular tables)."""
    nA, nB = len(degrees), max(degrees)
    ei = np.concatenate([np.full(d, k) for k, d in enumerate(degrees)])
    ej = np.concatenate([nA + (k + np.arange(d)) % nB for k, d in enumerate(degrees)])
    return mrf([L] * nA + [leaf_L or L] * nB, ei, ej, pairwise, seed, compute_primal)


def hub_position(n_spokes, hub_at) -> int:
    return {"first": 0, "middle": n_spokes // 2, "last": n_spokes}.get(hub_at, hub_at)


def star(L, pairwise, n_spokes, hub_at, seed=1, compute_primal=False) -> M.FlatModel:
    """one hub with ``n_spokes`` neighbours and nothing else; ``hub_at``: "first" (all the hub's ops are sends in the forward sweep,
    receives in the backward one), "last" (the reverse), "middle" (an even split), or the hub's index = its earlier neighbours"""
    h = hub_position(n_spokes, hub_at)
    v = np.array([x for x in range(n_spokes + 1) if x != h])
    return mrf([L] * (n_spokes + 1), np.minimum(h, v), np.maximum(h, v), pairwise, seed, compute_primal)


def banded(L, offsets, n, pairwise="dense", seed=3, compute_primal=False) -> M.FlatModel:
    """variables 0 .. n-1 in index order, an edge (i, i + o) for every offset (banded_model of tests/test_mailbox_gpu.py): n levels
    per sweep, every record away from the two ends with len(offsets) receives and as many sends in an anisotropic mode"""
    ei = np.concatenate([np.arange(0, n - o) for o in offsets]); ej = np.concatenate([np.arange(0, n - o) + o for o in offsets])
    return mrf([L] * n, ei, ej, pairwise, seed, compute_primal)


def pw_dup(L, sched, dup, seed=1) -> M.FlatModel:
    """a chain u0 - p0 - u1 - p1 - u2 whose pairwise factors are updated (``sched``: SCHED_FULL / SCHED_RIGHT), the message of the left
    unary added 1 + ``dup`` times: 2 + dup messages per pairwise factor, each received and sent in a uniform mode"""
    mt = [M.MsgType(0, 1, sched, 0, 0, M.M_UNARY_PAIRWISE, 0), M.MsgType(0, 1, sched, 0, 0, M.M_UNARY_PAIRWISE, 1)]
    rng = np.random.default_rng(seed)
    b = M.ModelBuilder(2, mt)
    u = b.add_vector_factors(0, rng.uniform(0, 1, (3, L)))
    for k in range(2):
        p = b.add_dense_pairwise(1, rng.uniform(0, 1, (1, L, L)))[0]
        b.add_messages(0, u[k], p); b.add_messages(1, u[k + 1], p)
        for _ in range(dup):
            b.add_messages(0, u[k], p)
        b.add_relations(u[k], p); b.add_relations(p, u[k + 1])
    return b.finish()


def grid(H, W, L, seed=1, compute_primal=False) -> M.FlatModel:
    return S.grid_model(H, W, L, order="colour_major", seed=seed, compute_primal=compute_primal)


def rect_chain(d0, d1, seed=1, compute_primal=False) -> M.FlatModel:
    """three variables with d0, d1, d0 labels in a chain: a d0 x d1 and a d1 x d0 table"""
    return mrf([d0, d1, d0], [0, 1], [1, 2], "dense", seed, compute_primal)


# ---- the case list -----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    """``kind``: dense / potts / shared (unaries updated) or pairwise (pw_dup); ``exact``: an exact class (4, 8, 16 or 32 labels on
    square tables), else run-time dims; ``cls``: the class the records run on while they fit; ``at_cap``: some record of some sweep
    has exactly cap ops and stays"""
    name: str
    family: str
    kind: str
    cls: str
    exact: bool
    at_cap: bool
    _build: Callable = dataclasses.field(repr=False, default=None)
    n_chain: Optional[int] = None                  # banded: ops per record in an anisotropic mode

    def model(self, compute_primal=False) -> M.FlatModel:
        return self._build(compute_primal)

    @property
    def cap(self) -> int:
        return class_cap(self.cls)


def class_of(pairwise, L, leaf_L=None) -> str:
    w = slot(max(L, leaf_L or L))
    if pairwise == "shared":
        return "shared%d" % w
    return "%s%s%d" % (pairwise, "" if (L in WIDTHS and leaf_L in (None, L)) else "_v", w)


def cap_degrees(cap, past=True):
    """the degrees of the hubs of a hub_side case; ``past`` False: nothing beyond the cap (a cap of 8 drops the 9 as well)"""
    deg = [1, 4, 8, 9, cap - 1, cap, cap, cap + 1, 2]
    return deg if past else [d for d in deg if d <= cap]


def _hub_cases():
    out = []
    def add(pairwise, L, past, leaf_L=None):
        cls = class_of(pairwise, L, leaf_L)
        deg = cap_degrees(class_cap(cls), past)
        name = "hubs %s %d%s labels %s" % (pairwise, L, "x%d" % leaf_L if leaf_L else "", "past cap" if past else "at cap")
        seed = 1000 + 10 * L + (leaf_L or 0) + (500 if past else 0)
        # (run-time dims past the cap: the hubs' launch leaves as a whole, nothing of the class is left at the cap)
        out.append(Case(name, "hub_side", pairwise, cls, "_v" not in cls and pairwise != "shared", "_v" not in cls or not past,
                        lambda cp=False: hub_side(L, pairwise, deg, leaf_L, seed, cp)))
    for pairwise in ("dense", "potts"):
        for L in WIDTHS:
            add(pairwise, L, True)
        for L in VAR_LABELS.values():             # the whole launch follows one record past the cap: both variants
            add(pairwise, L, False); add(pairwise, L, True)
    add("dense", 5, False, 7); add("dense", 5, True, 7)       # rectangular, both sides below the padded width 8
    for L in (4, 8, 16, 32, 21):
        add("shared", L, True)
    return out


# every hub position at cap - 1, cap, cap + 1: the exact classes, and one class each of the run-time-dims and shared ones
FULL_STARS = [(pw, L) for pw in ("dense", "potts") for L in WIDTHS] + [("dense", 5), ("potts", 21), ("shared", 16)]


def _star_cases():
    out = []
    def add(pairwise, L, n_spokes, hub_at, at_cap):
        cls = class_of(pairwise, L)
        name = "star %s %d labels %d spokes hub %s" % (pairwise, L, n_spokes, hub_at)
        out.append(Case(name, "star", pairwise, cls, "_v" not in cls and pairwise != "shared", at_cap,
                        lambda cp=False: star(L, pairwise, n_spokes, hub_at, 2000 + 100 * L + n_spokes, cp)))
    reps = [(pw, L) for pw in ("dense", "potts") for L in WIDTHS + tuple(VAR_LABELS.values())] + [("shared", L) for L in (4, 8, 16, 21)]
    for pairwise, L in reps:
        cap = class_cap(class_of(pairwise, L))
        add(pairwise, L, cap // 2, "middle", True)        # at the cap in the uniform modes: cap / 2 receives AND sends
        add(pairwise, L, cap, "middle", True)
        add(pairwise, L, cap, 3, True)                    # 3 receives (odd) and cap - 3 > 4 sends in the forward sweep; the reverse backward
        add(pairwise, L, cap + 1, "middle", False)
        if (pairwise, L) in FULL_STARS:
            add(pairwise, L, cap - 1, "middle", False)
            for hub_at in ("first", "last"):
                for n_spokes in (cap - 1, cap, cap + 1):
                    add(pairwise, L, n_spokes, hub_at, n_spokes == cap)
    return out


# (pairwise, labels, k): offsets 1 .. k, 2 k ops per full record in an anisotropic mode
BANDED = [("dense", 8, 8), ("dense", 16, 32), ("dense", 32, 16), ("dense", 5, 8), ("dense", 8, 5), ("potts", 16, 16)]
CHAIN_MIN_LAUNCHES = 9                               # plan.hpp: shorter schedules run as plain launches


def banded_n(k) -> int:
    """the smallest n with two FULL records (k earlier and k later neighbours: variables k and k + 1) — never fewer levels than a
    chain needs (tests/test_op_caps_host.py asserts that such a model plans as one chain launch)"""
    return max(2 * k + 2, CHAIN_MIN_LAUNCHES)


def _banded_cases():
    out = []
    for pairwise, L, k in BANDED:
        cls = class_of(pairwise, L)
        n = banded_n(k)
        out.append(Case("banded %s %d labels offsets 1..%d" % (pairwise, L, k), "banded", pairwise, cls, "_v" not in cls, 2 * k == class_cap(cls),
                        lambda cp=False, pairwise=pairwise, L=L, k=k, n=n: banded(L, range(1, k + 1), n, pairwise, 3000 + L + k, cp), n_chain=2 * k))
    return out


MIXED_CHAIN = dict(L=8, n=40, k=4, hub=10, far=8)


def mixed_chain(L, n, k, hub, far, seed=3500, compute_primal=False) -> M.FlatModel:
    """banded with offsets 1 .. k (2 k <= PK_MAX_OPS ops: packets) and ``far`` more edges from variable ``hub`` to hub + k + 1 ...:
    ONE chain launch whose levels are packet launches, indirect launches of 2 k + 1 ops and one indirect launch at the cap
    (k + (k + far) ops at ``hub``) — the stride changes from ticket to ticket"""
    off = range(1, k + 1)
    ei = np.concatenate([np.arange(0, n - o) for o in off] + [np.full(far, hub)])
    ej = np.concatenate([np.arange(0, n - o) + o for o in off] + [hub + k + 1 + np.arange(far)])
    return mrf([L] * n, ei, ej, "dense", seed, compute_primal)


def _mixed_cases():
    g = MIXED_CHAIN
    assert 2 * g["k"] + g["far"] == DENSE_CAP[g["L"]] and 2 * g["k"] <= PK_MAX_OPS
    return [Case("mixed chain dense %d labels" % g["L"], "mixed_chain", "dense", class_of("dense", g["L"]), True, True,
                 lambda cp=False: mixed_chain(compute_primal=cp, **g), n_chain=DENSE_CAP[g["L"]])]


def _pw_cases():
    out = []
    for L in (3, 8, 16, 21):
        for sched, sname in ((M.SCHED_FULL, "full"), (M.SCHED_RIGHT, "right")):
            for dup in (1, 2):
                cls = "small" if 2 * L <= SMALL_MAXD else "pairwise%d" % slot(L)
                out.append(Case("pw_dup %d labels %s dup %d" % (L, sname, dup), "pw_dup", "pairwise", cls, False, dup == 1 and cls != "small",
                                lambda cp=False, L=L, sched=sched, dup=dup: pw_dup(L, sched, dup, 4000 + L + dup)))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _hub_cases() + _star_cases() + _banded_cases() + _mixed_cases() + _pw_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


def case(name) -> Case:
    (c,) = [c for c in cases() if c.name == name]
    return c


def family(name):
    return [c for c in cases() if c.family == name]


# the limits (not part of the census): name -> builder(compute_primal)
BIG_LABELS = (320, 321, 384, 449, 512)
RECT_SIDES = ((512, 1), (1, 512), (512, 33), (33, 512), (300, 512))
LIMITS = {"star 2 labels 32767 spokes": lambda cp=False: star(2, "dense", MAX_ACTIVE, "middle", 5000, cp),
          "star 2 labels 32768 spokes": lambda cp=False: star(2, "dense", MAX_ACTIVE + 1, "middle", 5001, cp),
          "star 40 labels 300 spokes": lambda cp=False: star(40, "dense", 300, "middle", 5002, cp)}
LIMITS.update({"grid 2x2 %d labels" % L: (lambda cp=False, L=L: grid(2, 2, L, 5100 + L, cp)) for L in BIG_LABELS})
LIMITS.update({"chain %dx%d" % s: (lambda cp=False, s=s: rect_chain(s[0], s[1], 5200 + s[0] + 2 * s[1], cp)) for s in RECT_SIDES})


# ---- what the planner must make of a sweep, from the caps above ----------------------------------------------------------------
@dataclasses.dataclass
class Sweep:
    """the records of one directional sweep: per update of ``Plan.update_order`` its factor, active receives and sends, level"""
    factor: np.ndarray
    n_recv: np.ndarray
    n_send: np.ndarray
    level: np.ndarray
    om_off: np.ndarray
    mk_off: np.ndarray

    @property
    def ops(self):
        return self.n_recv + self.n_send


def sweep(plan, d, mode) -> Sweep:
    """from Plan.update_order / Plan.omega / Plan.mask / Plan.update_levels alone"""
    oo, om = plan.omega(d, mode); mo, mk = plan.mask(d, mode)
    count = lambda off, act: np.diff(np.concatenate([[0], np.cumsum(act)])[off])
    return Sweep(plan.update_order(d), count(mo, mk != 0).astype(np.int64), count(oo, om != 0).astype(np.int64), plan.update_levels(d, mode), oo, mo)


def widths(m: M.FlatModel) -> np.ndarray:
    """per factor: the largest label count of the factor and of any side of a table it is the left of a message to"""
    w = np.maximum(m.f_dim0, m.f_dim1).astype(np.int64)
    np.maximum.at(w, m.m_left, np.maximum(m.f_dim0, m.f_dim1)[m.m_right])
    return w


def expected_record_classes(c: Case, m: M.FlatModel, s: Sweep):
    """(base, final): per update the class it runs on while it fits its slab, and the class the caps above send it to (None: no op, no
    record).  Exact classes: only the records past the cap move, to dense_big.  Run-time-dims classes: the whole launch (the records
    of one level and class) follows ONE record past the cap to dense_big.  Shared: the record alone to small / generic.  Updated
    pairwise: the record alone to generic."""
    assert c.kind != "pairwise"
    w = widths(m)[s.factor]
    ops = s.ops
    base = np.empty(ops.shape[0], object); final = np.empty(ops.shape[0], object)
    for i in range(ops.shape[0]):
        if ops[i] == 0:
            base[i] = final[i] = None
        elif w[i] > 32:
            base[i] = final[i] = "dense_big"
        elif c.kind == "shared":
            base[i] = "shared%d" % slot(w[i])
            final[i] = base[i] if ops[i] <= class_cap(base[i]) else "small" if w[i] <= SMALL_MAXD else "generic"
        else:
            base[i] = "%s%s%d" % (c.kind, "" if c.exact else "_v", slot(w[i]))
            final[i] = base[i] if ops[i] <= class_cap(base[i]) else "dense_big"
    if not c.exact and c.kind != "shared":
        for lv, b in {(int(lv), b) for lv, b in zip(s.level, base) if b is not None and b != "dense_big"}:
            sel = np.array([s.level[i] == lv and base[i] == b for i in range(ops.shape[0])])
            if np.any(ops[sel] > class_cap(b)):
                final[sel] = "dense_big"
    return base, final


def split(final) -> dict:
    out = {}
    for f in final:
        if f is not None:
            out[f] = out.get(f, 0) + 1
    return out


def expected_pairwise_split(c: Case, m: M.FlatModel, s: Sweep):
    """pw_dup: {class: records}.  The updated PAIRWISE factors: within PW_MAX_OPS ops the packed pairwise class of the padded width,
    past it generic; tables whose two message vectors fit SMALL_MAXD doubles run one lane each whatever their ops.  The unaries
    (updated under SCHED_FULL only): u0 and u1 have two messages into ONE vector, which the packed kernels do not run — one lane
    each up to SMALL_MAXD labels, else the streaming class; u2 is an ordinary record of its dense class."""
    L = int(m.f_dim0[0])
    out = {}
    for f, ops in zip(s.factor, s.ops):
        if ops == 0:
            continue
        if m.f_kind[f] != M.F_VECTOR:
            k = c.cls if c.cls == "small" or ops <= PW_MAX_OPS else "generic"
        elif np.sum(m.m_left == f) > 1:
            k = "small" if L <= SMALL_MAXD else "dense_big"
        else:
            k = class_of("dense", L)
        out[k] = out.get(k, 0) + 1
    return out


# ---- census ------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Census:
    """``cells[(class, ops)]``: the set of (n_recv, n_send, "aniso" / "uniform") of the records that RUN on the class with that many
    ops; ``moved[(class, ops)]``: where records of the class's shape with that many ops run instead; ``crowded``: classes with a
    launch (one level of one sweep) of two or more records at the cap next to records below it; ``chain[(class, ops)]``: banded
    cases whose records have that many ops inside the one chain launch of the forward sweep"""
    cells: dict
    moved: dict
    crowded: set
    chain: dict


def census(case_list, plan_of: Callable) -> Census:
    """``plan_of(model)``: the planner (lp_mp_amd.engine.Plan; passed in so that this module stays plain numpy)"""
    cen = Census({}, {}, set(), {})
    for c in case_list:
        m = c.model()
        p = plan_of(m)
        for d in DIRECTIONS:
            for mode in MODES:
                s = sweep(p, d, mode)
                kind = "aniso" if mode in ANISO_MODES else "uniform"
                if c.kind == "pairwise":
                    for f, r, sd in zip(s.factor, s.n_recv, s.n_send):
                        if m.f_kind[f] == M.F_VECTOR or r + sd == 0 or c.cls == "small":
                            continue
                        if r + sd <= PW_MAX_OPS:
                            cen.cells.setdefault((c.cls, int(r + sd)), set()).add((int(r), int(sd), kind))
                        else:
                            cen.moved.setdefault((c.cls, int(r + sd)), set()).add("generic")
                    continue
                base, final = expected_record_classes(c, m, s)
                for i in range(base.shape[0]):
                    if base[i] is None:
                        continue
                    key = (base[i], int(s.ops[i]))
                    if final[i] == base[i]:
                        cen.cells.setdefault(key, set()).add((int(s.n_recv[i]), int(s.n_send[i]), kind))
                    else:
                        cen.moved.setdefault(key, set()).add(final[i])
                for b in set(final) - {None, "dense_big", "small", "generic"}:
                    for lv in set(s.level[final == b].tolist()):
                        o = s.ops[(final == b) & (s.level == lv)]
                        if np.sum(o == class_cap(b)) >= 2 and np.any(o < class_cap(b)):
                            cen.crowded.add(b)
                if c.family == "banded" and d == M.FORWARD and mode == M.REPAM_ANISOTROPIC:
                    cen.chain[(c.cls, c.n_chain)] = int(np.sum((final == c.cls) & (s.ops == c.n_chain)))
    return cen


def census_gaps(cen: Census) -> list:
    """what the list would leave untested (empty: the census is complete).  Every packed class runs records with 8, 9, cap - 1 and cap
    ops (those within its cap) and has cap + 1 moved away; at the cap: fewer and more than 4 sends (the prefetched ones), an odd and
    an even number of receives, an anisotropic and a uniform mode; a crowded launch.  Every reachable packed pairwise class at
    PW_MAX_OPS, with 8 ops moved to generic.  The chain executor: every banded shape."""
    gaps = []
    for k in PACKED_CLASSES:
        cap = class_cap(k)
        for ops in sorted({8, 9, cap - 1, cap}):
            if ops <= cap and (k, ops) not in cen.cells:
                gaps.append((k, ops, "never runs"))
        if not cen.moved.get((k, cap + 1)) or k in cen.moved.get((k, cap + 1)):
            gaps.append((k, cap + 1, "not moved away"))
        at = cen.cells.get((k, cap), set())
        for what, ok in (("fewer than 4 sends", any(0 < sd < 4 for _, sd, _ in at)), ("more than 4 sends", any(sd > 4 for _, sd, _ in at)),
                         ("odd receives", any(r % 2 == 1 for r, _, _ in at)), ("even receives", any(r % 2 == 0 for r, _, _ in at)),
                         ("anisotropic", any(q == "aniso" for _, _, q in at)), ("uniform", any(q == "uniform" for _, _, q in at))):
            if not ok:
                gaps.append((k, cap, what))
        if k not in cen.crowded:
            gaps.append((k, cap, "no crowded launch"))
    for k in PAIRWISE_CLASSES:
        if (k, PW_MAX_OPS) not in cen.cells:
            gaps.append((k, PW_MAX_OPS, "never runs"))
        if cen.moved.get((k, 8)) != {"generic"}:
            gaps.append((k, 8, "not moved to generic"))
    for pairwise, L, n_off in BANDED:
        if cen.chain.get((class_of(pairwise, L), 2 * n_off), 0) < 2:
            gaps.append((class_of(pairwise, L), 2 * n_off, "not in a chain"))
    return gaps
