"""Pairwise factors that round themselves (MPLP-style models: a COMPUTE_PRIMAL pairwise type under a `full` / `right` message
schedule) on every pairwise kind, storage mode and kernel class: the case list of tests/test_pairwise_rounding_host.py
and tests/test_pairwise_rounding_gpu.py, the numpy statement of the rounding rule, and the census of the kernel classes a case
reaches.

Every case is a pair (model, yardstick model): the yardstick is the expansion to private dense tables (expand_diff / expand_shared,
with_f32_tables for float storage), which the CPU oracle runs.  The rule below is written from the hook semantics quoted in
oracle/lpmp_oracle.c (primal rounding inside the sweep) and evaluates the cost on the KIND (readout_cases.cost_table), never on the
expansion.  Models are built once per process and never modified."""
import dataclasses
import functools

import numpy as np

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import readout_cases as RC

MODES = (M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2, M.REPAM_UNIFORM, M.REPAM_DAMPED_UNIFORM)
KINDS = ("dense", "dense_f32", "potts", "shared", "diff", "diff_band", "diff_shift", "mixed")
SCHEDS = {"full": M.SCHED_FULL, "right": M.SCHED_RIGHT}
# (schedule, computes): computes = (0, 1): only the pairwise factors round; (1, 1): the unaries round too and keep what a pairwise
# factor gave them
COMBOS = (("full", (0, 1)), ("right", (1, 1)), ("full", (1, 1)), ("right", (0, 1)))
VALUES = ("u01", "quant", "zero", "inf")
ORDERS = ("row_major", "colour_major")
# label counts by the class the updated pairwise factor takes in plain passes and the kernel it takes in primal passes
SMALL = ((3, 3), (4, 4), (2, 6))                       # d0 + d1 <= 8: lane per factor, plain and primal passes
PACKED = ((5, 5), (8, 8), (16, 16), (32, 32), (5, 7))  # pairwise4 ... 32: rerouted to the generic kernel in primal passes
GENERIC = ((33, 33), (40, 40), (70, 70), (20, 45))
BIG = ((128, 128), (256, 256), (200, 312))             # d0 + d1 up to GEN_MAXD = 512 (DIFF kinds and dense f64 only)
REFUSED = (257, 256)                                   # d0 + d1 = 513: set_reparametrization refuses the model
INF = float("inf")


# ---- models --------------------------------------------------------------------------------------------------------------------
def mtypes(sched, flags=0):
    return [M.MsgType(0, 1, sched, 0, 1, M.M_UNARY_PAIRWISE, 0, flags), M.MsgType(0, 1, sched, 0, 1, M.M_UNARY_PAIRWISE, 1, flags)]


def build(unaries, edges, sched, computes, flags=0):
    """Variables 0 .. n-1 in variable order (factor ids 0 .. n-1), one pairwise factor per edge (factor id n + e).  ``edges``:
    (i, j, spec) with variable i on side 0 and j on side 1; i or j None: no message on that side (a factor with a unary on one
    side only).  spec: ("dense", T) | ("potts", c) | ("shared", V, scale) | ("diff", D, scale) | ("shift", D, scale, shift) — arrays
    that are the same object share one pool entry.  Relations unary -> pairwise -> unary.  ``flags``: the MF_* flags of both
    message types (MF_IMPROVEMENT: the op the adaptive send rule asks for its weights)."""
    b = M.ModelBuilder(2, mtypes(sched, flags), list(computes))
    u = [int(b.add_vector_factors(0, np.asarray(c, np.float64)[None])[0]) for c in unaries]
    pool = {}

    def entry(a, vec):
        if id(a) not in pool:
            pool[id(a)] = b.add_diff_table(a) if vec else b.add_shared_table(a)
        return pool[id(a)]
    for i, j, spec in edges:
        k = spec[0]
        if k == "dense":
            p = int(b.add_dense_pairwise(1, np.asarray(spec[1], np.float64))[0])
        elif k == "potts":
            p = int(b.add_potts_pairwise(1, spec[2], [spec[1]])[0])
        elif k == "shared":
            p = int(b.add_shared_pairwise(1, [entry(spec[1], False)], [spec[2]])[0])
        elif k == "diff":
            p = int(b.add_diff_pairwise(1, spec[3][0], spec[3][1], [entry(spec[1], True)], [spec[2]])[0])
        else:
            assert k == "shift", k
            p = int(b.add_diff_shift_pairwise(1, spec[4][0], spec[4][1], [entry(spec[1], True)], [spec[2]], [spec[3]])[0])
        if i is not None:
            b.add_messages(0, [u[i]], [p]); b.add_relations(u[i], p)
        if j is not None:
            b.add_messages(1, [u[j]], [p]); b.add_relations(p, u[j])
    return b.finish()


class _Vals:
    """the value axis: u01 costs; costs quantised to {0, 0.5, 1} with every scale 1 (restricted minima tie); all zero; u01 with
    about 10 % +inf entries, a finite entry kept in every row and column of every expansion"""

    def __init__(self, values, seed):
        self.values, self.rng = values, np.random.default_rng(seed)

    def draw(self, shape):
        if self.values == "zero":
            return np.zeros(shape)
        x = self.rng.uniform(0, 1, shape)
        return np.round(x * 2.0) / 2.0 if self.values == "quant" else x

    def holes(self, x, keep):
        if self.values != "inf":
            return x
        hole = (self.rng.uniform(size=x.shape) < 0.1) & ~keep
        if not hole.any() and not keep.all():          # (a short vector: at least one hole where one may be)
            hole.reshape(-1)[np.flatnonzero(~keep.reshape(-1))[0]] = True
        x = x.copy()
        x[hole] = INF
        return x

    def scale(self, negative=False):
        if self.values in ("quant", "zero"):
            return 1.0
        if negative and self.values == "u01":
            return -0.75
        return float(self.rng.uniform(0.5, 2.0))


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def edge_spec(kind, d0, d1, e, v, pools):
    """the pairwise factor of edge number e of a model of one kind; ``pools``: the model's pooled tables / vectors by (kind,
    dims)"""
    Lm = max(d0, d1)
    if kind == "potts" and d0 != d1:          # (the mixed model only: its dense part is float-valued)
        kind = "dense_f32"
    if kind in ("dense", "dense_f32"):
        keep = np.zeros((d0, d1), bool)
        keep[np.arange(d0), np.arange(d0) % d1] = True
        keep[np.arange(d1) % d0, np.arange(d1)] = True
        T = v.holes(v.draw((d0, d1)), keep)
        return ("dense", _f32(T) if kind == "dense_f32" else T)
    if kind == "potts":
        c = {"zero": 0.0, "quant": float(v.rng.choice([-0.5, 0.5, 1.0]))}.get(v.values)
        return ("potts", float(v.rng.uniform(-0.5, 1.0)) if c is None else c, d0)
    if kind == "shared":
        key = ("shared", d0, d1)
        if key not in pools:
            keep = np.zeros((d0, d1), bool)
            keep[np.arange(d0), np.arange(d0) % d1] = True
            keep[np.arange(d1) % d0, np.arange(d1)] = True
            pools[key] = [v.holes(v.draw((d0, d1)), keep) for _ in range(2)]
        return ("shared", pools[key][e % 2], v.scale(negative=e == 1))
    if kind == "diff":
        key = ("diff", d0, d1)
        if key not in pools:
            assert v.values != "inf" or d0 == d1, "+inf vectors: square factors only (the entry of a == b stays finite)"
            keep = np.zeros(d0 + d1 - 1, bool)
            keep[d1 - 1] = True
            pools[key] = [v.holes(v.draw(d0 + d1 - 1), keep) for _ in range(2)]
        return ("diff", pools[key][e % 2], v.scale(negative=e == 1), (d0, d1))
    if kind == "diff_band":
        # truncated linear: min(slope * |a - b|, trunc), the truncation reached at |a - b| = T: a band of 2 T - 1 entries
        key = ("band", d0, d1)
        if key not in pools:
            T = 1 if Lm < 16 else 3
            trunc = (1.0, 1.0) if v.values == "quant" else (0.0, 0.0) if v.values == "zero" else (0.3, 0.45)
            pools[key] = [M.truncated_linear(d0, d1, t / T, t) for t in trunc]
            if v.values == "quant" and d0 + d1 - 1 >= 12:
                # quantised: a pooled potential that repeats values INSIDE its band — 0 at |a - b| = r, 0.5 between, 1 in the
                # tails (r = 2 where the vector has 20 entries, 1 below; under 12 entries the band rule leaves room for one entry
                # only) — so that minima tie across different differences, not along one diagonal only
                r = 2 if d0 + d1 - 1 >= 20 else 1
                k = np.abs(np.arange(d0 + d1 - 1) - (d1 - 1))
                pools[key] = [np.where(k == r, 0.0, np.where(k < r, 0.5, 1.0)) for _ in range(2)]
            assert all(M.diff_band_is_banded(x) for x in pools[key]), (d0, d1)
        return ("diff", pools[key][e % 2], v.scale(), (d0, d1))
    assert kind == "diff_shift", kind
    key = ("shift", d0, d1)
    if key not in pools:
        if v.values == "inf":           # lengths <= min(d0, d1): a row or column holds the whole vector or, clamped, one end of it
            assert d0 == d1
            lens = (min(5, Lm), Lm, max(3, Lm // 2))
        else:
            lens = (5, Lm, 2 * Lm - 1)
        vecs = []
        for n in lens:
            keep = np.zeros(n, bool)
            keep[[0, n // 2, n - 1]] = True
            vecs.append(v.holes(v.draw(n), keep))
        pools[key] = vecs
    D = pools[key][e % 3]
    n = D.shape[0]
    # shifts: random in [-(n + L), n + L]; 0; d1 - 1 (the plain DIFF shift where n = d0 + d1 - 1); indices clamped at the low
    # end for about half of the table; ... at the high end
    r = e % 6
    s = (0, d1 - 1, -(Lm // 2), n - 1 + Lm // 2)[r - 1] if 1 <= r <= 4 else int(v.rng.integers(-(n + Lm), n + Lm + 1))
    return ("shift", D, v.scale(negative=e == 1), s, (d0, d1))


def grid_edge_list(H, W, order):
    var = S.grid_variable_order(H, W, order).reshape(-1)
    a, bb = S.grid_edges(H, W)
    return [(int(min(var[x], var[y])), int(max(var[x], var[y]))) for x, y in zip(a, bb)]


MIXED_KINDS = ("dense_f32", "potts", "shared", "diff", "diff_band", "diff_shift", "shared")


def structure(struct, d0, d1):
    """(dims per variable, [(i, j)]) — i on side 0, j on side 1, None: no unary on that side"""
    name = struct[0]
    if name == "grid":
        _, H, W, order = struct
        assert d0 == d1
        return [d0] * (H * W), grid_edge_list(H, W, order)
    if name == "chain":                       # label counts d0, d1, d0, ...: factors d0 x d1 and d1 x d0 in turn
        n = struct[1] + 1
        return [d0 if k % 2 == 0 else d1 for k in range(n)], [(k, k + 1) for k in range(n - 1)]
    if name == "star":                        # 5 leaves of d1 labels round a centre of d0: the centre on either side
        return [d1, d1, d0, d1, d1, d1], [(0, 2), (1, 2), (2, 3), (2, 4), (2, 5)]
    if name == "one_sided":                   # a 3-chain, one factor with a unary on side 1 only, one with a unary on side 0 only
        return [d0, d1, d0], [(0, 1), (1, 2), (None, 2), (0, None)]
    if name == "pairs":                       # separate factors with two unaries of their own: each rounds with BOTH sides free
        n = struct[1]
        return [d0 if k % 2 == 0 else d1 for k in range(2 * n)], [(2 * k, 2 * k + 1) for k in range(n)]
    if name == "hub":                         # every kind in one neighbourhood: variable 0 next to all, a few edges between them
        return ([d0, d1, d0, d1, d0, d0, d1, d0],
                [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (1, 2), (2, 3), (3, 4), (5, 6), (6, 7)])
    raise ValueError(name)


@dataclasses.dataclass(frozen=True)
class Case:
    kind: str
    d0: int
    d1: int
    struct: tuple
    sched: str
    computes: tuple
    values: str = "u01"
    seed: int = 1
    flags: int = 0          # MF_* flags of the message types (0 for every case of the list)

    @property
    def name(self):
        s = "x".join(str(x) for x in self.struct)
        n = "%s-%dx%d-%s-%s-%d%d-%s" % (self.kind, self.d0, self.d1, s, self.sched, self.computes[0], self.computes[1], self.values)
        return n + ("-flags%d" % self.flags if self.flags else "")

    @property
    def precision(self):
        """the table precision of the engine that runs the case"""
        return "f32" if self.kind in ("dense_f32", "mixed") else None

    @property
    def model(self):
        return _model(self)

    @property
    def yardstick(self):
        return _yardstick(self)


@functools.lru_cache(maxsize=None)
def _model(c):
    v = _Vals(c.values, 1000 * c.seed + 7 * c.d0 + c.d1)
    dims, pairs = structure(c.struct, c.d0, c.d1)
    pools, edges = {}, []
    for e, (i, j) in enumerate(pairs):
        # the dims of a side without a unary: those of the chain the factor hangs on (d1 x d0 under (None, 2), d0 x d1 under (0,
        # None))
        a = dims[i] if i is not None else (c.d1 if dims[j] == c.d0 else c.d0)
        bb = dims[j] if j is not None else (c.d1 if dims[i] == c.d0 else c.d0)
        kind = MIXED_KINDS[e % len(MIXED_KINDS)] if c.kind == "mixed" else c.kind
        edges.append((i, j, edge_spec(kind, a, bb, e, v, pools)))
    return build([v.draw(d) for d in dims], edges, SCHEDS[c.sched], c.computes, c.flags)


def oracle_model(m, precision=None):
    """the model the unchanged CPU oracle runs: DIFF / DIFF_SHIFT and SHARED factors expanded to private dense tables, the tables
    of the DENSE factors rounded to float first where the device stores floats (equal values on float-valued tables; the pooled
    kinds stay doubles on the device, so their expansions are not rounded)"""
    if precision:
        m = m.with_f32_tables()
    return m.expand_diff().expand_shared()


@functools.lru_cache(maxsize=None)
def _yardstick(c):
    return oracle_model(c.model, c.precision)


def _primary(kind, d0, d1, si):
    if d0 != d1:
        return ("chain", {(2, 6): 9, (5, 7): 6, (20, 45): 4, (200, 312): 3, (3, 4): 5}[(d0, d1)])
    if d0 <= 40:
        return ("grid", 5, 6, ORDERS[si % 2])
    return ("grid", 3, 4, "colour_major") if d0 == 70 else ("grid", 3, 3, "row_major")


def _cases():
    out = []
    for kind in KINDS:
        if kind == "mixed":
            for si, (d0, d1) in enumerate(((3, 4), (5, 7), (20, 45))):
                for sched, computes in COMBOS:
                    out.append(Case(kind, d0, d1, ("hub",), sched, computes, seed=si))
            for values in ("quant", "zero"):
                for k, (d0, d1) in enumerate(((3, 4), (5, 7))):
                    out.append(Case(kind, d0, d1, ("hub",), *COMBOS[k], values=values))
                    out.append(Case(kind, d0, d1, ("hub",), *COMBOS[k + 2], values=values))
            # +inf entries: a square chain through the kinds in turn (the DIFF kinds keep their finite entries on square
            # factors only; why a chain: below)
            for k, L in enumerate((8, 33)):
                for ci in (k, k + 2):
                    out.append(Case(kind, L, L, ("chain", 7), *COMBOS[ci], values="inf", seed=60 + k))
            continue
        shapes = SMALL + PACKED + GENERIC
        if kind in ("dense", "diff", "diff_shift"):
            shapes += BIG
        elif kind == "diff_band":
            shapes += BIG[:1]
        if kind == "potts":
            shapes = tuple(s for s in shapes if s[0] == s[1])
        for si, (d0, d1) in enumerate(shapes):
            every = (d0, d1) in ((8, 8), (40, 40), (5, 7))
            for ci, (sched, computes) in enumerate(COMBOS):
                if not every and ci % 2 != si % 2:
                    continue
                # the order of a grid: both orders at every shape (the two combinations a shape keeps differ in ci // 2)
                struct = _primary(kind, d0, d1, ci if every else si + ci // 2)
                out.append(Case(kind, d0, d1, struct, sched, computes, seed=si))
        # the structures that are no grid and no alternating chain: a star, factors with a unary on one side only, a square chain
        extra = (5, 5) if kind == "potts" else (5, 7)
        for ci, struct in enumerate((("star",), ("one_sided",), ("one_sided",), ("chain", 3))):
            dd = (3, 3) if ci == 2 else extra
            out.append(Case(kind, dd[0], dd[1], struct, *COMBOS[ci], seed=20 + ci))
            out.append(Case(kind, dd[0], dd[1], struct, *COMBOS[(ci + 2) % 4], seed=30 + ci))
        # quantised costs: ties are the rule; all zero: every minimiser is the first
        for k, (d0, d1) in enumerate(((4, 4), (8, 8), (40, 40), extra)):
            for ci in (k % 4, (k + 1) % 4, (k + 2) % 4):
                struct = _primary(kind, d0, d1, ci) if d0 != d1 or k < 3 else ("chain", 6)
                out.append(Case(kind, d0, d1, struct, *COMBOS[ci], values="quant", seed=40 + k))
        for k, (d0, d1) in enumerate(((8, 8), extra, (33, 33))):
            struct = _primary(kind, d0, d1, k + 1) if d0 != d1 or k != 1 else ("chain", 6)
            out.append(Case(kind, d0, d1, struct, *COMBOS[k], values="zero", seed=50 + k))
            out.append(Case(kind, d0, d1, struct, *COMBOS[(k + 2) % 4], values="zero", seed=50 + k))
        # +inf entries, on chains: a factor of a chain never finds both sides given, so it never has to take a +inf pair and every
        # rounding pass ends with a finite cost (on a grid the cost of a pass may be +inf: not wanted here)
        if kind not in ("potts", "diff_band"):                     # (a Potts scalar and a truncated-linear vector have no holes)
            for k, L in enumerate((8, 33)):
                for ci in (k, k + 2):
                    out.append(Case(kind, L, L, ("chain", 7), *COMBOS[ci], values="inf", seed=60 + k))
    # separate pairs, quantised: the tie order of the full d0 x d1 walk decides every label (in a connected model only the first
    # factor of a sweep has both sides free)
    for kind in KINDS:
        for k, (d0, d1, n) in enumerate(((5, 7, 14), (20, 45, 7)) if kind == "mixed" else ((8, 8, 12), (40, 40, 6))):
            out.append(Case(kind, d0, d1, ("pairs", n), *COMBOS[k], values="quant", seed=80 + k))
            out.append(Case(kind, d0, d1, ("pairs", n), *COMBOS[k + 2], values="quant", seed=80 + k))
    names = [c.name for c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def refused_model():
    """a 257 x 256 factor that is updated: d0 + d1 = 513 is one more than the generic kernel holds"""
    d0, d1 = REFUSED
    D = np.linspace(0.0, 1.0, d0 + d1 - 1)
    return build([np.zeros(d0), np.zeros(d1)], [(0, 1, ("diff", D, 1.0, (d0, d1)))], M.SCHED_FULL, (0, 1))


def per_kind(d0, d1=None, sched="full", computes=(1, 1)):
    """one case per kind at the given label counts (Potts and the mixed model at their nearest), for the once-per-kind tests"""
    d1 = d0 if d1 is None else d1
    out = []
    for kind in KINDS:
        pick = [c for c in CASES if c.kind == kind and c.values == "u01" and c.computes == computes and c.sched == sched and
                ((c.d0, c.d1) == (d0, d1) or (kind == "mixed" and (c.d0, c.d1) == ((5, 7) if d0 <= 8 else (20, 45))))]
        assert pick, (kind, d0, d1)
        out.append(pick[0])
    return out


# ---- the rule, restated in numpy -----------------------------------------------------------------------------------------------
def links(m):
    """(side_unary, of_unary): side_unary[(p, s)] = the unary on side s of pairwise factor p (absent: none); of_unary[u] = its
    (p, s) in message order"""
    side_unary, of_unary = {}, {}
    for k in range(m.n_messages):
        u, p, s = int(m.m_left[k]), int(m.m_right[k]), int(m.mtypes[int(m.m_type[k])].param)
        assert (p, s) not in side_unary
        side_unary[(p, s)] = u
        of_unary.setdefault(u, []).append((p, s))
    return side_unary, of_unary


def round_pairwise(m, coff, doff, duals, primal, p, side_unary, variant="first"):
    """One primal update of pairwise factor p from its duals after the receives, float64, explicit loops.  A side is given if its
    unary holds a label, else if the factor's own slot holds one; the free sides take the first minimiser, in row-major order, of
    cost(a, b) + m1[a] + m2[b] restricted to the given sides.  Returns (x0, x1, free0, free1).
    ``variant`` seeds a wrong rule: "last" (the last minimiser), "column_major" (tie order), "ignore_given" (both sides free)."""
    d0, d1 = int(m.f_dim0[p]), int(m.f_dim1[p])
    T = RC.cost_table(m, coff, p)                  # the cost on the kind itself
    m1 = duals[doff[p]: doff[p] + d0]
    m2 = duals[doff[p] + d0: doff[p] + d0 + d1]
    x = []
    for s, d in ((0, d0), (1, d1)):
        u = side_unary.get((p, s))
        lab = int(primal[u, 0]) if u is not None and primal[u, 0] < d else int(primal[p, s])
        x.append(lab if lab < d else None)
    if variant == "ignore_given":
        x = [None, None]
    free0, free1 = x[0] is None, x[1] is None
    if not (free0 or free1):
        return x[0], x[1], False, False
    ra = range(d0) if free0 else (x[0],)
    rb = range(d1) if free1 else (x[1],)
    best, arg = None, None
    pairs = ((a, b) for b in rb for a in ra) if variant == "column_major" else ((a, b) for a in ra for b in rb)
    for a, b in pairs:
        v = float(T[a, b]) + float(m1[a]) + float(m2[b])
        if best is None or v < best or (variant == "last" and v <= best):
            best, arg = v, (a, b)
    return arg[0], arg[1], free0, free1


def unset_primal(m):
    """init_primal of every factor: an unset entry holds the dimension"""
    pr = np.zeros((m.n_factors, 2), np.int32)
    pr[:, 0] = m.f_dim0
    pw = m.f_kind != M.F_VECTOR
    pr[pw, 1] = m.f_dim1[pw]
    return pr


def simulate_sweep(m, yard, d, mode, duals0, primal0, variant="first"):
    """The labels of one rounding sweep (direction d, weight mode) from the duals ``duals0`` and the labels ``primal0`` of the
    same time stamp, by the numpy rule.  The duals a factor rounds on — its state after its receives — come from the oracle's
    PLAIN update rule (rounding never changes a dual): the updates before it replayed from duals0, then its own with every send
    weight 0."""
    o = Oracle(yard)
    o.set_reparametrization(mode)
    upd = o.update_order(d)
    oo, om = o.omega(d, mode)
    mo, mk = o.mask(d, mode)
    side_unary, of_unary = links(m)
    doff, coff = m.dual_offsets(), m.const_offsets()
    primal = np.array(primal0, np.int32, copy=True)
    computes = m.ftype_computes_primal

    def label_unary(u, x):
        primal[u, 0] = x
        for p, s in of_unary.get(u, ()):
            primal[p, s] = x
    for k, f in enumerate(upd):
        f = int(f)
        if not computes[m.f_type[f]]:
            continue
        w = om[:oo[k + 1]].copy()
        w[oo[k]:] = 0.0
        o.set_duals(duals0)
        o.compute_pass_custom(upd[:k + 1], oo[:k + 2], w, mo[:k + 2], mk[:mo[k + 1]])
        dual = o.duals()
        if m.f_kind[f] == M.F_VECTOR:
            n = int(m.f_dim0[f])
            if primal[f, 0] >= n:
                best = 0
                for i in range(1, n):
                    if dual[doff[f] + i] < dual[doff[f] + best]:
                        best = i
                label_unary(f, best)
            continue
        x0, x1, free0, free1 = round_pairwise(m, coff, doff, dual, primal, f, side_unary, variant)
        primal[f, 0], primal[f, 1] = x0, x1
        for s, x, free in ((0, x0, free0), (1, x1, free1)):
            u = side_unary.get((f, s))
            if free and u is not None:
                label_unary(u, x)
    return primal


def energy(m, primal):
    """the energy of a labelling on the kind model's ORIGINAL costs (``m.dual_data`` holds the original unaries and zero messages):
    +inf when a label is unset"""
    doff, coff = m.dual_offsets(), m.const_offsets()
    e = float(m.constant)
    for f in range(m.n_factors):
        a = int(primal[f, 0])
        if m.f_kind[f] == M.F_VECTOR:
            if a >= m.f_dim0[f]:
                return INF
            e += float(m.dual_data[doff[f] + a])
        else:
            b = int(primal[f, 1])
            if a >= m.f_dim0[f] or b >= m.f_dim1[f]:
                return INF
            e += float(RC.cost_table(m, coff, f)[a, b])
    return e


def consistent_preset(m, labelled, rng):
    """a labelling with the unaries ``labelled`` (a bool per VECTOR factor, in factor order) holding random labels, every slot of a
    pairwise factor a copy of its unary's label, everything else unset"""
    pr = unset_primal(m)
    side_unary, of_unary = links(m)
    unaries = np.flatnonzero(m.f_kind == M.F_VECTOR)
    for u, on in zip(unaries, labelled):
        if on:
            x = int(rng.integers(0, m.f_dim0[u]))
            pr[u, 0] = x
            for p, s in of_unary.get(int(u), ()):
                pr[p, s] = x
    return pr


# ---- census --------------------------------------------------------------------------------------------------------------------
def pairwise_cell(name):
    return name if name in ("small", "generic") or name.startswith("pairwise") else "other:" + name


def census(c, probe_lib, mode=M.REPAM_ANISOTROPIC):
    """(classes, pairwise, unary): the kernel classes of both directions as Plan.schedule_classes counts them; the classes of the
    updated PAIRWISE records; the classes of the updated UNARY records, with "diff:banded" / "diff:shifted" where launches of class
    diff run the banded kernel / hold DIFF_SHIFT factors.  Per record, from the planner's own schedule (schedule_hazards.Probe)."""
    import schedule_hazards as H
    from collections import Counter
    m = c.model
    plan = E.Plan(m)
    o = Oracle(c.yardstick)
    o.set_reparametrization(mode)
    probe = H.Probe(probe_lib, m)
    classes, pairwise, unary = [], set(), set()
    for d in (M.FORWARD, M.BACKWARD):
        oo, om = o.omega(d, mode)
        mo, mk = o.mask(d, mode)
        S_ = probe.plan([(o.update_order(d), oo, om, mo, mk)], fuse=False)
        names = [E.KCLASS_NAMES[int(k)] for k in S_["rec_class"]]
        classes.append(plan.schedule_classes(d, mode))
        assert dict(Counter(names)) == classes[-1], (c.name, d)
        for f, n in zip(S_["rec_factor"], names):
            (pairwise if m.f_kind[int(f)] != M.F_VECTOR else unary).add(n)
        if "diff" in unary:
            info = plan.diff_band_info(d, mode)
            if info["band_launches"] > 0:
                unary.add("diff:banded")
            if np.any(m.f_kind == M.F_PAIRWISE_DIFF_SHIFT):
                unary.add("diff:shifted")
            if info["band_launches"] < info["diff_launches"] and np.any(m.f_kind == M.F_PAIRWISE_DIFF):
                unary.add("diff:plain")
    return classes, pairwise, unary
