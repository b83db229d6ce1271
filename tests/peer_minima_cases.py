"""Models for the peer-minima form of the joined passes beyond the colour-major grid (kernels.hip dense_pq_*_body): bipartite
graphs in a 2-colour order whose records sit on EITHER side of their tables, with 1-4 edges in any order of insertion, parallel edges
and isolated unaries.  No GPU and no pytest here: the builders, the case list and a census of it from the edge lists alone.

Terms.  Colour 0 is inserted first and holds the consuming records (H, K, T), colour 1 last and holds the publishing ones (W).  The SIDE
of a unary on an edge is the side of the edge's table its labels index: 0 the rows (the unary is the left of message type 0), 1 the
columns (type 1).  An edge is FLIPPED when its colour-1 unary is on side 0; ``synthetic.grid_model(order="colour_major")`` flips none.
The planner lists a factor's messages type by type (plan.cpp), so a record's receives (and sends) are the edges it is on side 0 of, then
those it is on side 1 of, each group in the order of the edge list: a record of mixed sides always has a side-0 table first."""
import dataclasses
from typing import Callable, Optional

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

L = 32
GRIDS = [(1, 7), (3, 3), (13, 11), (14, 10), (40, 36)]
MAX_DEGREE = 4                                    # plan.hpp PEER_MINIMA_MAX_OPS: receives (and sends) of a record of the form


def bipartite_model(n0, n1, edges, flip, side1_first, L=L, seed=1, tables=None) -> M.FlatModel:
    """``n0`` colour-0 unaries, one dense pairwise factor per row (a, b) of ``edges`` (a < n0, b < n1), ``n1`` colour-1 unaries, inserted in
    that order, relations u0[a] -> pw[e] -> u1[b].  Edge e not flipped: u0[a] is the left of message type 0 (side 0, the table's rows)
    and u1[b] the left of type 1; flipped: the other way round.  ``side1_first[e]``: the side-1 message of e is added before the
    side-0 one.  Costs are uniform(0, 1), the tables random per edge (never symmetric), or ``tables`` [E, L, L]."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    flip = np.asarray(flip, bool); side1_first = np.asarray(side1_first, bool)
    E = edges.shape[0]
    assert flip.shape == (E,) and side1_first.shape == (E,)
    assert E == 0 or (edges.min() >= 0 and edges[:, 0].max() < n0 and edges[:, 1].max() < n1)
    rng = np.random.default_rng(seed)
    un0, un1 = rng.uniform(0, 1, (n0, L)), rng.uniform(0, 1, (n1, L))
    if tables is None:
        tables = rng.uniform(0, 1, (E, L, L))
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u0 = b.add_vector_factors(0, un0)
    pw = b.add_dense_pairwise(1, np.asarray(tables, np.float64).reshape(E, L, L))
    u1 = b.add_vector_factors(0, un1)
    a, c = u0[edges[:, 0]], u1[edges[:, 1]]
    on0, on1 = np.where(flip, c, a), np.where(flip, a, c)              # the unary on side 0 / side 1 of every edge
    mt = np.empty(2 * E, np.int32); left = np.empty(2 * E, np.int32); right = np.repeat(pw, 2).astype(np.int32)
    mt[0::2] = np.where(side1_first, 1, 0); mt[1::2] = np.where(side1_first, 0, 1)
    left[0::2] = np.where(side1_first, on1, on0); left[1::2] = np.where(side1_first, on0, on1)
    b.add_interleaved_messages(mt, left, right, return_ids=False)
    f1 = np.empty(2 * E, np.int32); f2 = np.empty(2 * E, np.int32)
    f1[0::2] = a; f2[0::2] = pw; f1[1::2] = pw; f2[1::2] = c
    b.add_relations(f1, f2)
    return b.finish()


@dataclasses.dataclass
class Case:
    """a model of the list and the graph it was built from: ``edges`` [E, 2] (a of colour 0, b of colour 1, each counted within its
    colour) in the order the messages were added, ``flip`` [E]; ``model(tables)`` builds it, with other tables where given (the
    row of ``tables`` for edge e is the table of pairwise factor ``pairwise(e)``)"""
    name: str
    family: str
    n0: int
    n1: int
    edges: np.ndarray
    flip: np.ndarray
    side1_first: np.ndarray
    _build: Callable = dataclasses.field(repr=False, default=None)
    _pw_first: int = 0

    def model(self, tables: Optional[np.ndarray] = None) -> M.FlatModel:
        return self._build(tables)

    def pairwise(self, e: int) -> int:
        return self._pw_first + int(e)

    def tables(self) -> np.ndarray:
        """the case's own tables [E, L, L], a copy"""
        m = self.model()
        off = m.const_offsets()[self.pairwise(0)]
        return np.array(m.const_data[off: off + self.edges.shape[0] * L * L], np.float64).reshape(-1, L, L)

    def graph_text(self) -> str:
        """what tests/cpp/*_probe.cpp read: ``n0 n1``, then an edge per line"""
        return "%d %d\n" % (self.n0, self.n1) + "".join("%d %d\n" % (a, b) for a, b in self.edges)


def _bipartite_case(name, family, n0, n1, edges, flip, side1_first, seed) -> Case:
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    flip = np.asarray(flip, bool); side1_first = np.asarray(side1_first, bool)
    return Case(name, family, n0, n1, edges, flip, side1_first,
                lambda tables=None: bipartite_model(n0, n1, edges, flip, side1_first, L, seed, tables), n0)


def colour_major_graph(H, W):
    """(n0, n1, edges) of the H x W grid: colour 0 the nodes with r + c even, both colours numbered in row-major order, the edges in
    the order of synthetic.grid_edges"""
    var = S.grid_variable_order(H, W, "colour_major").reshape(-1)
    a, b = S.grid_edges(H, W)
    n0 = (H * W + 1) // 2
    va, vb = var[a], var[b]
    return n0, H * W - n0, np.stack([np.minimum(va, vb), np.maximum(va, vb) - n0], 1)


def suggested_order_case(H, W, seed) -> Case:
    """the README's workflow: the grid inserted row by row, Plan.suggest_order, with_factor_order.  Edges are (i, i + 1) / (i, i + W) in
    row-major numbering with the lower node on side 0, so the side of the publishing record alternates from edge to edge."""
    from lp_mp_amd import engine as E                                   # (the planner: native, host only)
    m = S.grid_model(H, W, L, order="row_major", seed=seed)
    rank, colours = E.Plan(m).suggest_order(0)
    assert colours == 2, colours
    n = H * W
    a, b = S.grid_edges(H, W)                                          # a < b; unary v = factor v, edge e = factor n + e, u_a on side 0
    first = rank[:n] < rank[n:].max()                                   # colour 1: the unaries behind every pairwise factor
    assert np.all(first[a] != first[b]) and np.all(rank[n:] > np.minimum(rank[a], rank[b])), "not a 2-colour order around the pairwise factors"
    idx = np.empty(n, np.int64)                                        # position of a unary within its colour, by rank
    for col in (first, ~first):
        v = np.flatnonzero(col)
        idx[v[np.argsort(rank[:n][v])]] = np.arange(v.shape[0])
    flip = ~first[a]
    edges = np.stack([np.where(flip, idx[b], idx[a]), np.where(flip, idx[a], idx[b])], 1)

    def build(tables=None):
        return S.grid_model(H, W, L, order="row_major", seed=seed, tables=tables).with_factor_order(rank)
    return Case("suggested %dx%d" % (H, W), "suggested", int(first.sum()), int(n - first.sum()), edges, flip, np.zeros(len(a), bool), build, n)


def thinned_graph(H, W, rng, keep=0.6, dup=0.3, every_unary_keeps_an_edge=False):
    """the colour-major grid graph with about ``keep`` of its edges, about ``dup`` of the survivors doubled (parallel edges) where
    both ends stay within MAX_DEGREE, in shuffled order.  Unaries may lose every edge unless ``every_unary_keeps_an_edge``."""
    n0, n1, edges = colour_major_graph(H, W)
    E = edges.shape[0]
    deg = [np.bincount(edges[:, 0], minlength=n0), np.bincount(edges[:, 1], minlength=n1)]
    alive = np.ones(E, bool)
    for e in rng.permutation(E):
        if alive.sum() <= round(keep * E):
            break
        a, b = edges[e]
        if every_unary_keeps_an_edge and (deg[0][a] < 2 or deg[1][b] < 2):
            continue
        alive[e] = False; deg[0][a] -= 1; deg[1][b] -= 1
    out = [tuple(x) for x in edges[alive]]
    for a, b in list(out):
        if rng.random() < dup and deg[0][a] < MAX_DEGREE and deg[1][b] < MAX_DEGREE:
            out.append((a, b)); deg[0][a] += 1; deg[1][b] += 1
    out = np.asarray(out, np.int64)[rng.permutation(len(out))]
    return n0, n1, out


def random_bipartite_graph(n0, n1, rng, attempts):
    """random pairs, kept where both ends stay within MAX_DEGREE (parallel edges as they come)"""
    deg = [np.zeros(n0, np.int64), np.zeros(n1, np.int64)]
    out = []
    for _ in range(attempts):
        a, b = int(rng.integers(n0)), int(rng.integers(n1))
        if deg[0][a] < MAX_DEGREE and deg[1][b] < MAX_DEGREE:
            out.append((a, b)); deg[0][a] += 1; deg[1][b] += 1
    return n0, n1, np.asarray(out, np.int64)


def star_graph(centres, leaves):
    """``centres`` colour-1 unaries with ``leaves`` colour-0 leaves each"""
    return centres * leaves, centres, np.asarray([(c * leaves + i, c) for c in range(centres) for i in range(leaves)], np.int64)


_CASES = None


def cases():
    """the case list (built once; the suggested-order cases ask the planner)"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    for H, W in GRIDS:
        out.append(suggested_order_case(H, W, seed=500 + H * W))
    for H, W in GRIDS:
        n0, n1, e = colour_major_graph(H, W)
        out.append(_bipartite_case("flipped %dx%d" % (H, W), "flipped", n0, n1, e, np.ones(len(e), bool), np.zeros(len(e), bool), 600 + H * W))
    for H, W in GRIDS:
        n0, n1, e = colour_major_graph(H, W)
        rng = np.random.default_rng(700 + H * W)
        out.append(_bipartite_case("random-flip %dx%d" % (H, W), "random-flip", n0, n1, e, rng.random(len(e)) < 0.5, rng.random(len(e)) < 0.5, 700 + H * W))
    for H, W, bound_rows in ((13, 11, False), (40, 36, False), (14, 10, True)):
        rng = np.random.default_rng(800 + H * W)
        n0, n1, e = thinned_graph(H, W, rng, every_unary_keeps_an_edge=bound_rows)
        out.append(_bipartite_case("thinned %dx%d" % (H, W), "thinned-connected" if bound_rows else "thinned", n0, n1, e,
                                   rng.random(len(e)) < 0.5, rng.random(len(e)) < 0.5, 800 + H * W))
    rng = np.random.default_rng(900)
    n0, n1, e = random_bipartite_graph(61, 45, rng, attempts=260)
    out.append(_bipartite_case("bipartite 61+45", "bipartite", n0, n1, e, rng.random(len(e)) < 0.5, rng.random(len(e)) < 0.5, 900))
    n0, n1, e = star_graph(3, 4)
    out.append(_bipartite_case("stars 3x4", "bipartite", n0, n1, e, rng.random(len(e)) < 0.5, rng.random(len(e)) < 0.5, 901))
    _CASES = out
    return out


def case(name) -> Case:
    (c,) = [c for c in cases() if c.name == name]
    return c


CASE_NAMES = (["suggested %dx%d" % g for g in GRIDS] + ["flipped %dx%d" % g for g in GRIDS] + ["random-flip %dx%d" % g for g in GRIDS] +
              ["thinned 13x11", "thinned 40x36", "thinned 14x10", "bipartite 61+45", "stars 3x4"])
FAMILIES = ("suggested", "flipped", "random-flip", "thinned", "thinned-connected", "bipartite")


# ---- census: which kinds of record the list holds, from the edge lists alone -------------------------------------------------
def record_sides(c: Case):
    """(publishing, consuming): for every record with an edge, the sides it is on, in the order of its receives (side 0 first)"""
    pub = [[] for _ in range(c.n1)]; con = [[] for _ in range(c.n0)]
    for (a, b), f in zip(c.edges, c.flip):
        con[a].append(1 if f else 0)
        pub[b].append(0 if f else 1)
    return [sorted(s) for s in pub if s], [sorted(s) for s in con if s]


def _pattern(sides):
    return "side 0" if not any(sides) else "side 1" if all(sides) else "mixed"


def census(c: Case) -> dict:
    """counts of records per cell: (role, edges, side pattern) for role in "publish" / "consume", and for publishing records with 3 and 4
    edges ("publish", edges, "receive 0" / "receive 1", side) — receive 0 is the table parked in LDS, receive 1 the one kept (3 edges)
    or requested twice (4); and ("consume", "wave", "sides differ"): pairs of consuming records that share a wave of the wide form
    (records 2 i and 2 i + 1 of the step, isolated unaries have none) and differ in side pattern"""
    out = {}
    pub, con = record_sides(c)
    differ = sum(1 for i in range(0, len(con) - 1, 2) if _pattern(con[i]) != _pattern(con[i + 1]))
    if differ:
        out[("consume", "wave", "sides differ")] = differ
    for role, recs in (("publish", pub), ("consume", con)):
        for s in recs:
            assert 1 <= len(s) <= MAX_DEGREE, (c.name, role, s)
            k = (role, len(s), _pattern(s))
            out[k] = out.get(k, 0) + 1
            if role == "publish" and len(s) >= 3:
                for j in (0, 1):
                    k = (role, len(s), "receive %d" % j, s[j])
                    out[k] = out.get(k, 0) + 1
    return out


def census_cells():
    """every cell that can exist (one edge cannot be mixed)"""
    cells = [(role, d, p) for role in ("publish", "consume") for d in range(1, MAX_DEGREE + 1) for p in ("side 0", "side 1", "mixed") if not (d == 1 and p == "mixed")]
    cells += [("publish", d, "receive %d" % j, s) for d in (3, 4) for j in (0, 1) for s in (0, 1)]
    cells += [("consume", "wave", "sides differ")]
    return cells
