"""Far offsets: a small live model behind tens of thousands of isolated padding factors, so that every constant and dual offset
the planner hands the kernels lies past 2^31 (placement P31) or 2^32 (P32) elements.  Helpers of tests/test_far_offsets_host.py
and tests/test_far_offsets_gpu.py.

The padding factors have no message: they are never updated, appear in no record, and contribute 0.0 to every bound (their
constants and duals are zero).  The far model has no host costs: they live in two caller-owned device tensors, zero in front and
the small model's packed arrays at the tail.  The oracle only ever sees the small model."""
import dataclasses
import functools

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

PAD_LABELS = 65536
N_PAD = {"P31": 32768, "P32": 65536}
TAIL = 1 << 22                 # doubles behind the padding: room for the largest live model of the tests (40 x 36 x 32: 2.9 M constants)
GIB = 1 << 30


def pad_sizes(n_pad, kind):
    """(const elements, dual elements) of the padding = the first live const / dual offset"""
    if kind == "dense":
        return n_pad * PAD_LABELS, n_pad * (PAD_LABELS + 1)
    if kind == "vector":
        return 0, n_pad * PAD_LABELS
    raise ValueError(kind)


def _pad_type(m, kind):
    """a factor type for the padding: one whose factors do not round a primal (those get a record without any message);
    kind dense: the type of m's pairwise factors where there is one"""
    cp = np.asarray(m.ftype_computes_primal)
    want = (m.f_kind != M.F_VECTOR) if kind == "dense" else (m.f_kind == M.F_VECTOR)
    for t in list(dict.fromkeys(int(t) for t in m.f_type[want])) + list(range(m.n_ftypes)):
        if not cp[t]:
            return t
    raise ValueError("pad_front: every factor type rounds a primal")


def pad_front(m, n_pad, kind="dense"):
    """``m`` with n_pad isolated factors in front: DENSE 1 x 65536 factors of the pairwise type (65 536 constants and 65 537 duals
    each) or VECTOR factors of 65 536 labels (duals only).  No host costs: upload with ``const_dev=`` / ``dual_dev=``."""
    n_pad = int(n_pad)
    pad_sizes(n_pad, kind)
    t = _pad_type(m, kind)
    front = lambda a, v: np.ascontiguousarray(np.concatenate([np.full(n_pad, v, a.dtype), a]))
    shift = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.int32) + np.int32(n_pad))
    dense = kind == "dense"
    return dataclasses.replace(
        m, _keep=[], const_data=None, dual_data=None,
        f_type=front(m.f_type, t), f_kind=front(m.f_kind, M.F_PAIRWISE_DENSE if dense else M.F_VECTOR), f_flags=front(m.f_flags, 0),
        f_dim0=front(m.f_dim0, 1 if dense else PAD_LABELS), f_dim1=front(m.f_dim1, PAD_LABELS if dense else 0),
        f_table=None if m.f_table is None else front(np.asarray(m.f_table, np.int32), -1),
        m_left=shift(m.m_left), m_right=shift(m.m_right), rel_fwd=shift(m.rel_fwd), rel_bwd=shift(m.rel_bwd),
        part_pairs=shift(m.part_pairs) if m.part_pairs is not None and len(m.part_pairs) else m.part_pairs)


class FarBuffers:
    """the two borrowed device tensors of one placement: ``torch.zeros(pad + TAIL)`` each, allocated once; ``load`` writes a small
    model's packed arrays behind the padding, ``reset`` zeroes what the last test used of the tails"""

    def __init__(self, placement, kind="dense"):
        import torch
        self.torch = torch
        self.placement, self.kind, self.n_pad = placement, kind, N_PAD[placement]
        self.pad_c, self.pad_d = pad_sizes(self.n_pad, kind)
        self.const = torch.zeros(self.pad_c + TAIL, dtype=torch.float64, device="cuda")
        self.dual = torch.zeros(self.pad_d + TAIL, dtype=torch.float64, device="cuda")
        self.n_c = self.n_d = 0
        torch.cuda.synchronize()

    @staticmethod
    def bytes_needed(placement, kind="dense"):
        c, d = pad_sizes(N_PAD[placement], kind)
        return 8 * (c + d + 2 * TAIL)

    def load(self, m, const=None, dual=None):
        """the tails := m.const_data / m.dual_data (or the arrays given); returns (const pointer, dual pointer)"""
        torch = self.torch
        const = m.const_data if const is None else const
        dual = m.dual_data if dual is None else dual
        assert const.shape[0] <= TAIL and dual.shape[0] <= TAIL
        self.reset()
        self.n_c, self.n_d = int(const.shape[0]), int(dual.shape[0])
        self.write_const(const)
        self.dual[self.pad_d: self.pad_d + self.n_d].copy_(torch.from_numpy(np.ascontiguousarray(dual, np.float64)))
        torch.cuda.synchronize()
        return self.const.data_ptr(), self.dual.data_ptr()

    def write_const(self, const):
        """the const tail rewritten in place (same length)"""
        n = int(const.shape[0])
        assert n == self.n_c
        if n:
            self.const[self.pad_c: self.pad_c + n].copy_(self.torch.from_numpy(np.ascontiguousarray(const, np.float64)))
        self.torch.cuda.synchronize()

    def reset(self):
        if self.n_c:
            self.const[self.pad_c: self.pad_c + self.n_c].zero_()
        if self.n_d:
            self.dual[self.pad_d: self.pad_d + self.n_d].zero_()
        self.n_c = self.n_d = 0
        self.torch.cuda.synchronize()

    def dual_tail(self):
        self.torch.cuda.synchronize()
        return self.dual[self.pad_d: self.pad_d + self.n_d].cpu().numpy()

    def const_tail(self):
        self.torch.cuda.synchronize()
        return self.const[self.pad_c: self.pad_c + self.n_c].cpu().numpy()

    def _nonzero_bits(self, t, n):
        """words of the first n doubles that are not +0.0 (by their bits: a -0.0 counts)"""
        return int(self.torch.count_nonzero(t[:n].view(self.torch.int64)).item()) if n else 0

    def dual_padding_nonzero(self):
        self.torch.cuda.synchronize()
        return self._nonzero_bits(self.dual, self.pad_d) + self._nonzero_bits(self.dual[self.pad_d + self.n_d:], TAIL - self.n_d)

    def const_padding_nonzero(self):
        self.torch.cuda.synchronize()
        return self._nonzero_bits(self.const, self.pad_c) + self._nonzero_bits(self.const[self.pad_c + self.n_c:], TAIL - self.n_c)


# ---- the live models: the smallest that still reach each kernel family ------------------------------------------------------
def _grid(L, pairwise="dense", shape=(6, 5), order="colour_major", **kw):
    return S.grid_model(shape[0], shape[1], L, pairwise=pairwise, order=order, seed=100 + L, **kw)


def _mixed():
    import diff_tables_cases as DT
    return DT.mixed_graph(np.random.default_rng(311), n=30)


def _diff40():
    import diff_tables_cases as DT
    return DT.label_grid(40, "colour_major")


def _band130():
    import diff_band_cases as DB
    return DB.label_grid(130, "colour_major", 2)


def _scheduled(sched):
    import f32_tables_cases as FC
    return FC.scheduled_grid(6, 5, 8, sched, 8 + sched)


def _level_loop():
    import diff_tables_cases as DT
    return DT.updated_pairwise_grid(M.SCHED_RIGHT, 40)     # row-major, updated DIFF factors: many tiny generic levels


def _c5():
    import recost_cases as RC
    return RC.c5_small()


def _diff_shift(L):
    import diff_shift_cases as DS
    return DS.label_grid(L, "colour_major")


def _diff_shift_mixed():
    import diff_shift_cases as DS
    return DS.mixed_graph(np.random.default_rng(311))       # DIFF_SHIFT beside DIFF, SHARED, DENSE and POTTS peers


def _diff_shift_band(L):
    import diff_shift_band_cases as DB
    return DB.label_grid(L, "colour_major")     # every vector with constant tails inside the rule: every shifted launch is banded


def _pq_mixed_sides():
    import peer_minima_cases as PQ
    return PQ.case(PQ_MIXED_SIDES).model()


def _labeling(name):
    import labeling_cases as LC
    return LC.case(name)


PQ_MIXED_SIDES = "random-flip 13x11"        # publishing and consuming records on both sides of their tables
# labeling lists whose left factor has several labelings: a case of the lane-per-factor class whose level loop takes the
# "paired staged" and the "staged" body, and one of the wave-per-factor class with nine left labelings
LABELING_NL = {"labeling_nl_small": "pair_trip7 chain full io11", "labeling_nl_generic": "gen9x20 chain full io01"}


# name -> (builder, the kernel classes the forward sweep must consist of under ANISOTROPIC; None: only "something generic")
LIVE = {
    "dense32": (lambda: _grid(32), {"dense32"}),
    "dense8": (lambda: _grid(8), {"dense8"}),
    "dense4": (lambda: _grid(4), {"dense4"}),
    "dense_v21": (lambda: _grid(21), {"dense_v32"}),
    "dense_v5": (lambda: _grid(5), {"dense_v8"}),
    "potts16": (lambda: _grid(16, "potts"), {"potts16"}),
    "potts_v5": (lambda: _grid(5, "potts"), {"potts_v8"}),
    "big48": (lambda: _grid(48, shape=(4, 4)), {"dense_big"}),
    "big130": (lambda: _grid(130, shape=(4, 4)), {"dense_big"}),
    "shared32": (lambda: _grid(32, "shared", n_tables=2), {"shared32"}),
    "shared8": (lambda: _grid(8, "shared", n_tables=2), {"shared8"}),
    "diff40": (_diff40, {"diff"}),
    "diff_band130": (_band130, {"diff"}),
    "pairwise8_right": (lambda: _scheduled(M.SCHED_RIGHT), None),
    "pairwise8_full": (lambda: _scheduled(M.SCHED_FULL), None),
    "mixed_graph": (_mixed, None),
    "c5_small": (_c5, None),
    "level_loop40": (_level_loop, None),
    "joined_dense32": (lambda: _grid(32, shape=(40, 36)), {"dense32"}),
    "joined_potts8": (lambda: _grid(8, "potts", shape=(64, 48)), {"potts8"}),
    "deep_dense16": (lambda: S.grid_model(40, 30, 16, order="row_major", seed=5), {"dense16"}),
    "deep_potts8": (lambda: S.grid_model(60, 50, 8, pairwise="potts", order="row_major", seed=6), {"potts8"}),
    "halo16": (lambda: _grid(16), {"dense16"}),
    "halo40": (lambda: _grid(40), {"dense_big"}),
    "primal_dense8": (lambda: _grid(8, compute_primal=True), {"dense8"}),
    "primal_potts8": (lambda: _grid(8, "potts", compute_primal=True), {"potts8"}),
    "recost13": (lambda: _grid(13, shape=(7, 6)), {"dense_v16"}),
    "diff_shift40": (lambda: _diff_shift(40), {"diff"}),
    "diff_shift130": (lambda: _diff_shift(130), {"diff"}),          # more than 64 labels: several registers per lane in a move
    "diff_shift_mixed": (_diff_shift_mixed, None),
    "pq_mixed_sides": (_pq_mixed_sides, {"dense32"}),
    # (`full` schedules: both sweeps update factors.  Their classes, "small" and "generic" alone, are pinned in
    # tests/test_far_offsets_host.py: these classes have no packets, which a class set named here would make the probe test ask for)
    "labeling_nl_small": (lambda: _labeling(LABELING_NL["labeling_nl_small"]), None),
    "labeling_nl_generic": (lambda: _labeling(LABELING_NL["labeling_nl_generic"]), None),
    "diff_shift_band40": (lambda: _diff_shift_band(40), {"diff"}),
    "diff_shift_band130": (lambda: _diff_shift_band(130), {"diff"}),        # more than 128 labels: the LDS-bound occupancy branch
    # the smallest grid of the skewed tiled order's near tests (tests/test_pq_ahead_gpu.py "24x24", tests/test_pq_tiles_gpu.py)
    "skew_dense32": (lambda: S.grid_model(24, 24, 32, order="colour_major", seed=9100 + 24 * 24), {"dense32"}),
}
DIFF_SHIFT_BAND_MODELS = ("diff_shift_band40", "diff_shift_band130")
DIFF_SHIFT_MODELS = ("diff_shift40", "diff_shift130", "diff_shift_mixed")
# the first three families of the issue's table: placement P32 as well
P32_MODELS = ("dense32", "dense8", "dense4", "dense_v21", "dense_v5", "potts16", "potts_v5", "big48", "big130")


def _shift24():
    import primal_state_cases as PS
    return PS.shift_model(PS.SHIFT_KEYS[0])


# live models that no sweep test runs (they are in none of the host module's lists over LIVE): the DIFF_SHIFT model of the label write-in
EXTRA = {"primal_shift24": _shift24}


@functools.lru_cache(maxsize=None)
def live(name):
    """built once per process and never modified"""
    return (LIVE[name][0] if name in LIVE else EXTRA[name])()


def oracle_model(m):
    """what the unchanged CPU oracle runs: DIFF and SHARED factors expanded to private tables"""
    return m.expand_diff().expand_shared()


# ---- path and forest moves: live models that come with their groups -----------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Relabel:
    """``make()`` -> (model, groups); upload keywords; passes before the move (0: random duals of seed ``duals``, written into the
    borrowed tail); the seed of the starting labelling"""
    make: object
    kw: tuple = ()
    passes: int = 2
    duals: int = 0
    start: int = 7


def _paths(name, *a, **kw):
    import path_moves_cases as PM
    return lambda: getattr(PM, name)(*a, **kw)


def _forest(name, *a, **kw):
    import forest_moves_cases as FM
    return lambda: getattr(FM, name)(*a, **kw)


def _thinned():
    import forest_moves_cases as FM
    from lp_mp_amd import engine as E
    m = FM.thinned_grid()
    return m, E.Plan(m).suggest_forests()


F32 = (("table_precision", "f32"),)
T7 = (-1, 0, 0, 1, 1, 1, 2)                     # forest_moves_cases.TREE7
PATH_CASES = {
    "dense13": Relabel(_paths("ladder", (13, 13, 13, 13), "dense", seed=3)),                  # f64 tables, both sides of an edge, the wave form
    "dense_f32": Relabel(_paths("ladder", (13, 9, 13, 9), "dense_f32", seed=4), kw=F32),     # pw_cost's float branch
    "mixed": Relabel(_paths("mixed_path_case")),          # dense, Potts, SHARED, DIFF, banded DIFF as path edges and as off-path lines
    "diff_shift": Relabel(_paths("diff_shift_case")),     # the four-word cell
    "rect_both_forms": Relabel(_paths("rect_case"), passes=0, duals=1015),                   # both forms, both back-pointer widths
    "length300": Relabel(_paths("long_case")),            # PathRec::node_begin and the back-pointer walk over 300 far nodes
}
FOREST_CASES = {
    "tree": Relabel(_forest("tree_model")),               # TREE7, dense, mixed sides
    "rect": Relabel(_forest("rect_case"), passes=0, duals=1026),
    "fan40": Relabel(_forest("fan_case", 40)),            # the largest fan of tests/test_forest_moves_gpu.py
    "diff_shift": Relabel(_forest("diff_shift_tree")),
    "thinned_grid": Relabel(_thinned),                    # the suggested cover of a grid with parallel edges and isolated unaries
    "potts": Relabel(_forest("tree_model", T7, (13,) * 7, "potts", seed=6)),
    "shared": Relabel(_forest("tree_model", T7, (13, 7, 13, 7, 13, 7, 13), "shared", seed=7)),
    "diff": Relabel(_forest("tree_model", T7, (40, 33, 40, 33, 40, 33, 40), "diff", seed=8)),
    "dense_f32": Relabel(_forest("tree_model", T7, (13, 9, 13, 9, 13, 9, 5), "dense_f32", seed=4), kw=F32),
}
RELABEL = {"path": PATH_CASES, "forest": FOREST_CASES}
RELABEL_ROUNDS = 2
P32_RELABEL = {"path": ("dense13", "mixed"), "forest": ("tree", "diff_shift")}


@functools.lru_cache(maxsize=None)
def relabel_case(kind, name):
    """(model, groups, the model the device computes on: float tables rounded); built once per process and never modified"""
    c = RELABEL[kind][name]
    m, groups = c.make()
    return m, groups, (m.with_f32_tables() if c.kw else m)


def relabel_start(kind, name):
    import path_moves_cases as PM
    return PM.random_primal(relabel_case(kind, name)[0], RELABEL[kind][name].start)


def relabel_random_duals(kind, name):
    c = RELABEL[kind][name]
    return None if c.passes else np.random.default_rng(c.duals).random(relabel_case(kind, name)[0].dual_data.shape[0])


def relabel_reference(kind, name, duals, start, trace=None):
    import forest_moves_cases as FM
    import path_moves_cases as PM
    _, groups, ref = relabel_case(kind, name)
    fn = PM.path_moves_reference if kind == "path" else FM.forest_moves_reference
    return fn(ref, duals, start, groups, rounds=RELABEL_ROUNDS, trace=trace)


def relabel_members(kind, groups):
    if kind == "path":
        return sorted({int(u) for g in groups for p in g for u in p})
    return sorted({int(u) for un, _ in groups for u in un})


def far_groups(kind, groups, n_pad):
    """the groups of the small model with n_pad added to every member (a root's parent stays -1)"""
    if kind == "path":
        return [[[int(u) + n_pad for u in p] for p in g] for g in groups]
    return [(np.asarray(un, np.int32) + np.int32(n_pad), np.where(np.asarray(par) == -1, -1, np.asarray(par) + n_pad).astype(np.int32)) for un, par in groups]


# ---- carried labels: the four moves of the far window tests, each with the labelling it starts from ---------------------------
CARRY_MODELS = ("diff_shift40", "diff_shift130")


def window_moves(name):
    """(unaries, longest window, [(deltas, with costs, from device memory, labels)]): the moves of the far window test of
    tests/test_far_offsets_gpu.py — deltas with 0, +-1, 63, -64, L - 1, -L and L + 7 —, and per move a random labelling of the
    small model with every sixth unary unset"""
    import move_windows_cases as MW
    import primal_state_cases as PS
    m = live(name)
    us = MW.unaries(m)
    L = int(m.f_dim0[us].max())
    delta = MW.deltas(m.f_dim0[us], L)
    moves = ((delta, False, False), (-delta, False, True), (delta[::-1].copy(), True, False), (-delta[::-1], True, True))
    return us, L, [(dl, costs, dev, PS.random_primal(m, 40 + k, unset_every=6)) for k, (dl, costs, dev) in enumerate(moves)]


def checkerboard_moves(name):
    """two more moves, there (host) and back (device memory), that keep a model with a +inf-tailed vector feasible: one colour of
    the graph's two-colouring moves by one label, so that the shift of EVERY DIFF_SHIFT cell changes by +-1 — inside the band that
    diff_shift_band_cases.feasible_shift keeps on the diagonal"""
    import move_windows_cases as MW
    m = live(name)
    us = MW.unaries(m)
    ends = {}
    for k in range(m.n_messages):
        ends.setdefault(int(m.m_right[k]), []).append(int(m.m_left[k]))
    adj = {int(u): [] for u in us}
    for a, b in ends.values():
        adj[a].append(b); adj[b].append(a)
    colour, stack = {int(us[0]): 0}, [int(us[0])]
    while stack:
        v = stack.pop()
        for w in adj[v]:
            if w not in colour:
                colour[w] = 1 - colour[v]
                stack.append(w)
            assert colour[w] != colour[v], "not two-colourable"
    assert len(colour) == len(us), "not connected"
    delta = np.asarray([colour[int(u)] for u in us], np.int64)
    return [(delta, False, False, None), (-delta, False, True, None)]


# ---- the scalars in device memory: the models of the list-bound procedure -----------------------------------------------------
SCALAR_MODELS = ("dense8", "diff40", "mixed_graph")
SET_LABEL_MODELS = ("primal_dense8", "primal_shift24")
