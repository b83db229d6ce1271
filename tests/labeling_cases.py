"""Labeling-list models whose LEFT factor has several labelings (``labeling_message<LEFT, RIGHT, INDICES...>`` with nl > 1, index
tuples of several positions, right labelings that match no left one): the models of tests/test_labeling_shapes_host.py (why they
can tell a wrong kernel from a right one, and which kernel body runs each of them) and tests/test_labeling_shapes_gpu.py.

A FAMILY is a pair of labeling lists and the index tuples of its match tables (nl x nr: nl left, nr right labelings); a SHAPE is a
bipartite graph of left and right factors; a CASE is a family on a shape under one message schedule and one pair of
implicit-origin flags.  ``case(name)`` builds the FlatModel, ``CASES[name]`` holds what the census needs.

Two conditions keep the duals finite (reference labeling_list_factor.hxx:411-443), and every case meets them (asserted on the
host):
  (a) every left labeling is matched by at least one right labeling in every table: else its message entry is +inf;
  (b) the right factor has an implicit origin or, in every table, at least one unmatched labeling: else not_taken is +inf and the
      message -inf.
A family of 9 left and 8 right labelings cannot meet (a) (nine labelings, eight matches at most): it is no case; the host test
shows what its tables (``impossible_9x8_tables``) do to the duals, and 9 x 9 stands next to it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

from lp_mp_amd import model as M

GEN_MAXD = 512                                # csrc/kernels.hpp
LL_STAGE_RECS, LL_STAGE_OPS = 16, 16          # csrc/plan.hpp
MODES = (M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2, M.REPAM_UNIFORM, M.REPAM_DAMPED_UNIFORM)
SCHEDS = {"left": M.SCHED_LEFT, "right": M.SCHED_RIGHT, "full": M.SCHED_FULL, "only send": M.SCHED_ONLY_SEND}
COPIES = (1, 7, 8, 9, 15, 16, 17, 23)
CALLS = (("forward", 0), ("backward", 0), ("pass", 1), ("pass", 2), ("pass", 5))     # the calls of the device tests


def call(x, what, n):
    """one entry of CALLS on the oracle or on an engine"""
    oracle = hasattr(x, "ComputePass")
    if what == "pass":
        x.ComputePass(n) if oracle else x.compute_pass(n)
    elif what == "forward":
        x.ComputeForwardPass() if oracle else x.forward_pass()
    else:
        x.ComputeBackwardPass() if oracle else x.backward_pass()


@dataclass(frozen=True)
class Family:
    name: str
    left: tuple
    right: tuple
    indices: tuple            # one index tuple per match table
    cls: str                  # "small" (lane per factor) or "generic" (wave per factor)
    io: Tuple[bool, bool]     # the default implicit-origin flags (left, right)

    @property
    def nl(self):
        return len(self.left)

    @property
    def nr(self):
        return len(self.right)

    def tables(self) -> List[np.ndarray]:
        """table[r] = index of the left labeling the right labeling r shows at the index tuple, nl if none"""
        pos = {l: i for i, l in enumerate(self.left)}
        return [np.asarray([pos.get(tuple(r[i] for i in idx), self.nl) for r in self.right], np.int32) for idx in self.indices]


def _bits(v: int, B: int) -> tuple:
    return tuple((v >> (B - 1 - i)) & 1 for i in range(B))


def synthetic_family(name: str, nl: int, nr: int, n_tables: int, n_unmatched: int, cls: str, io=(False, True), seed: int = 0) -> Family:
    """bit codes: the left labelings are the B-bit codes of 0 .. nl - 1; a right labeling is one B-bit code per table (the entry the
    table shall hold for it; the code of nl stands for "unmatched") followed by the code of its own number, which no table reads and
    which keeps the labelings distinct.  Every table is onto 0 .. nl - 1 (condition a) and holds n_unmatched unmatched entries."""
    assert nr - n_unmatched >= nl
    rng = np.random.default_rng(77000 + seed)
    B, Br = max(1, int(nl).bit_length()), max(1, int(nr - 1).bit_length())
    ent = []
    for k in range(n_tables):
        e = np.concatenate([rng.permutation(nl), rng.integers(0, nl, nr - n_unmatched - nl), np.full(n_unmatched, nl)])
        ent.append(e[rng.permutation(nr)])
    left = tuple(_bits(v, B) for v in range(nl))
    right = tuple(sum((_bits(int(ent[k][r]), B) for k in range(n_tables)), ()) + _bits(r, Br) for r in range(nr))
    fam = Family(name, left, right, tuple(tuple(range(k * B, (k + 1) * B)) for k in range(n_tables)), cls, io)
    assert all(np.array_equal(t, e) for t, e in zip(fam.tables(), ent))
    return fam


def _all_bits(n):
    return tuple(_bits(v, n) for v in range(1 << n))


PAIRS3 = ((0, 1), (0, 2), (1, 2))
FAMILIES: Dict[str, Family] = {f.name: f for f in (
    # today's shape, the control: 1 x 4
    Family("edge_trip", ((1,),), ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1)), ((0,), (1,), (2,)), "small", (True, True)),
    # 3 x 7: the non-zero labelings of a pair of bits against those of three bits, every table with unmatched entries
    Family("pair_trip7", ((0, 1), (1, 0), (1, 1)), _all_bits(3)[1:], PAIRS3, "small", (True, True)),
    # 4 x 8: (0, 0) is a left labeling, every entry is matched, nr = SMALL_MAXD; the right factor needs its implicit origin (b)
    Family("pair4_trip8", _all_bits(2), _all_bits(3), PAIRS3, "small", (False, True)),
    # 8 x 8: right labelings (a, b, c, a); (0, 1, 2) reads the identity, (1, 2, 3) the non-monotone permutation (b, c, a)
    Family("perm8", _all_bits(3), tuple(b + (b[0],) for b in _all_bits(3)), ((0, 1, 2), (1, 2, 3)), "small", (False, True)),
    # 2 x 8: three right labelings per left one and two unmatched, in both tables
    Family("many_to_one", ((0,), (1,)), ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1)), ((0,), (1,)), "small", (False, False)),
    synthetic_family("gen3x9", 3, 9, 3, 2, "generic", seed=1),            # only the peer is too big for the lane-per-factor class
    synthetic_family("gen9x9", 9, 9, 2, 0, "generic", seed=2),            # the nearest family to 9 x 8 that meets (a)
    synthetic_family("gen9x20", 9, 20, 3, 3, "generic", seed=3),
    synthetic_family("gen64x130", 64, 130, 2, 5, "generic", seed=4),
    synthetic_family("gen65x200", 65, 200, 2, 7, "generic", seed=5),      # stride loops with a remainder of 1
    synthetic_family("gen200x512", 200, 512, 2, 30, "generic", seed=6),   # the right factor at GEN_MAXD
    synthetic_family("gen5x600", 5, 600, 2, 40, "generic", seed=7),       # the peer above GEN_MAXD, own size and len 5
)}
SMALL = [f for f in FAMILIES.values() if f.cls == "small"]
GENERIC = [f for f in FAMILIES.values() if f.cls == "generic"]


def impossible_9x8_tables(seed: int = 0) -> List[np.ndarray]:
    """9 left labelings, 8 right ones: whatever the tables hold, a left labeling stays unmatched (the host test shows the effect)"""
    rng = np.random.default_rng(seed)
    return [rng.permutation(9)[:8].astype(np.int32) for _ in range(2)]


# ---- shapes: (number of left factors, number of right factors, [(left, right, table)]) ------------------------------------------
def chain(n: int, T: int):
    """the right factor t joins the left factors t, t + 1, ... through tables 0, 1, ...: one record per level, n levels deep"""
    return n + T - 1, n, [(t + k, t, k) for t in range(n) for k in range(T)]


def copies(k: int, n: int, T: int):
    """k independent chains: k records per level"""
    nl_, nr_, e = chain(n, T)
    return k * nl_, k * nr_, [(c * nl_ + a, c * nr_ + b, t) for c in range(k) for a, b, t in e]


def hub(h: int, T: int, n: int = 10, at: int = 5):
    """a chain whose left factor ``at`` has h right neighbours in all (the extra ones joined through table 0 alone)"""
    nl_, nr_, e = chain(n, T)
    deg = sum(1 for a, _, _ in e if a == at)
    assert h >= deg
    return nl_, nr_ + h - deg, e + [(at, nr_ + x, 0) for x in range(h - deg)]


def dup(T: int, n: int = 10, at: int = 5):
    """a chain in which the left factor ``at`` is joined to the right factor ``at`` through table 0 AND table 1"""
    nl_, nr_, e = chain(n, T)
    assert (at, at, 0) in e and (at, at, 1) not in e
    return nl_, nr_, e + [(at, at, 1)]


def bipartite(T: int, seed: int, n_left: int = 14, n_right: int = 18):
    rng = np.random.default_rng(88000 + seed)
    e = []
    for r in range(n_right):
        for k, a in enumerate(rng.choice(n_left, T, replace=False)):
            e.append((int(a), r, k))
    return n_left, n_right, e


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    shape: str                # chain / copies<k> / hub<h> / dup / random
    sched: str
    io: Tuple[bool, bool]
    chain_min: int = 0        # LPMP_CHAIN_MIN the case needs to reach the chain executor (0: the default)
    seed: int = 0

    @property
    def fam(self) -> Family:
        return FAMILIES[self.family]

    def graph(self):
        T = len(self.fam.indices)
        if self.shape == "chain":
            return chain(10, T)
        if self.shape.startswith("copies"):
            return copies(int(self.shape[6:]), 4, T)
        if self.shape.startswith("hub"):
            return hub(int(self.shape[3:]), T)
        if self.shape == "dup":
            return dup(T)
        assert self.shape == "random"
        return bipartite(T, self.seed)


def build(c: Case, flags: int = 0, tables=None) -> M.FlatModel:
    """``flags``: MF_* of every message type (MF_IMPROVEMENT for the adaptive send rule); ``tables``: other match tables than the
    family's (same sizes: the host test's wrong tables)"""
    f = c.fam
    T = len(f.indices)
    b = M.ModelBuilder(2, [M.MsgType(0, 1, SCHEDS[c.sched], M.variableMessageNumber, M.variableMessageNumber, M.M_LABELING, k, flags) for k in range(T)])
    for k in range(T):
        b.add_labeling_table(f.left, f.right, f.indices[k])
    if tables is not None:
        assert all(t.shape == u.shape for t, u in zip(tables, b._tables))
        b._tables = [np.asarray(t, np.int32) for t in tables]
    n_left, n_right, edges = c.graph()
    rng = np.random.default_rng(99000 + c.seed)
    lf = b.add_vector_factors(0, rng.uniform(-1, 1, (n_left, f.nl)), implicit_origin=c.io[0])
    rf = b.add_vector_factors(1, rng.uniform(-1, 1, (n_right, f.nr)), implicit_origin=c.io[1])
    for a, r, k in edges:
        b.add_messages(k, lf[a], rf[r])
        b.add_relations(lf[a], rf[r])
    b.constant = 0.25
    return b.finish()


def _cases() -> Dict[str, Case]:
    out = []

    def add(fam, shape, sched="left", io=None, chain_min=0, seed=0):
        io = FAMILIES[fam].io if io is None else io
        out.append(Case("%s %s %s io%d%d" % (fam, shape, sched, io[0], io[1]), fam, shape, sched, io, chain_min, seed))
    for f in SMALL:
        for s in SCHEDS:
            add(f.name, "chain", s)
        add(f.name, "random", "left", chain_min=2, seed=len(out))
    for k in COPIES:
        add("pair_trip7", "copies%d" % k, chain_min=2)
        add("perm8", "copies%d" % k, chain_min=2)
    for k in (16, 17):
        add("many_to_one", "copies%d" % k, chain_min=2)
        add("pair4_trip8", "copies%d" % k, chain_min=2)
        add("edge_trip", "copies%d" % k, chain_min=2)          # the control on both sides of the staging limit
    for f in ("pair_trip7", "pair4_trip8", "perm8"):
        for h in (8, 9):
            add(f, "hub%d" % h)
    for f in ("pair_trip7", "many_to_one", "perm8"):
        add(f, "dup")
    add("pair_trip7", "random", "full", chain_min=2, seed=41)
    add("perm8", "random", "right", chain_min=2, seed=42)
    # all four combinations of the implicit-origin flags where the tables have unmatched entries (b)
    for f in ("edge_trip", "pair_trip7", "many_to_one"):
        for io in ((False, False), (False, True), (True, False), (True, True)):
            if io != FAMILIES[f].io:
                add(f, "chain", "left", io)
    for f in ("pair4_trip8", "perm8"):
        add(f, "chain", "left", (True, True))
    for f in GENERIC:
        if f.name == "gen200x512":          # under schedules that update the right factor
            add(f.name, "chain", "right")
            add(f.name, "chain", "full")
        else:
            add(f.name, "chain", "left")
    add("gen9x20", "chain", "full")
    add("gen9x20", "random", "only send", chain_min=2, seed=43)
    add("gen3x9", "random", "left", chain_min=2, seed=44)
    return {c.name: c for c in out}


CASES: Dict[str, Case] = _cases()
SMALL_CASES = [c for c in CASES.values() if c.fam.cls == "small"]
GENERIC_CASES = [c for c in CASES.values() if c.fam.cls == "generic"]


def case(name: str, flags: int = 0) -> M.FlatModel:
    return build(CASES[name], flags)


# ---- the census: which kernel body runs a case ---------------------------------------------------------------------------------
BODIES = ("paired staged", "staged", "paired", "plain", "lane per factor")


def bodies(plan, d: int, mode: int) -> Dict[str, int]:
    """launches of the sweep's level loop by the body of kernels.hip that runs them under the shared send rule:
    label_ops_body<PAIRED, STAGED>, label_ops_body_staged, label_ops_body<true>, label_ops_body<false>, generic_body<1>"""
    i = plan.level_loop_info(d, mode)
    ps, st, pr = i["label_paired_staged"], i["label_staged"], i["label_paired"]
    return dict(zip(BODIES, (ps, st - ps, pr - ps, i["label_ops"] - st - (pr - ps), i["lane_launches"] - i["label_ops"])))


ENGINES = (("level loop", {}), ("graph replay", {"LPMP_NO_LEVEL_LOOP": "1"}), ("chain tickets", {"LPMP_CHAIN_ALL": "1"}),
           ("plain launches", {"LPMP_NO_CHAIN": "1"}))


def assert_path(plan, c: Case, which: str):
    """the class split of both sweeps in every mode (no other class may stand in), and that a plan made under the environment of
    engine ``which`` takes the path the engine stands for (LPMP_NO_CHAIN is the engine's own switch: nothing of it is in a plan)"""
    for mode in MODES:
        n = 0
        for d in (M.FORWARD, M.BACKWARD):
            cls = plan.schedule_classes(d, mode)
            assert set(cls) <= {c.fam.cls}, (c.name, which, d, mode, cls)
            n += sum(cls.values())
        assert n > 0, (c.name, which, mode)
    ci, ll = plan.chain_info(M.BACKWARD, M.REPAM_UNIFORM), plan.level_loop_info(M.BACKWARD, M.REPAM_UNIFORM)
    if which == "graph replay":
        assert ci["n_chains"] == 0 and ll["launches"] == 0, (c.name, ci, ll)
    elif which == "chain tickets":
        assert ci["n_chains"] == 1 and ci["n_tickets"] > 0 and ll["launches"] == 0, (c.name, ci, ll)
    else:
        assert ci["n_chains"] == 1 and ci["n_tickets"] == 0 and ll["launches"] > 0, (c.name, ci, ll)
        assert ll["lane_launches"] == (ll["launches"] if c.fam.cls == "small" else 0), (c.name, ll)
