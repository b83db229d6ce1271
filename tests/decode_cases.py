"""Conditional rounding from the duals (lpmp_decode_primal): the numpy statement of the rule and the models of
tests/test_decode_host.py and tests/test_decode_gpu.py.  Written from the rule as include/lpmp_engine.h states it, not from the
device code.  Models are built once per process and never modified."""
import functools
import itertools

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

INF = float("inf")


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def structure(m):
    """(unaries, links): the VECTOR factors in factor order, and per unary its links (pairwise factor, side of the unary in it, the
    unary on the other side) in ascending message index.  Asserts the supported shape of the model."""
    side_unary = {}
    for k in range(m.n_messages):
        mt = m.mtypes[int(m.m_type[k])]
        assert mt.kind == M.M_UNARY_PAIRWISE
        key = (int(m.m_right[k]), int(mt.param))
        assert key not in side_unary
        side_unary[key] = int(m.m_left[k])
    unaries = [f for f in range(m.n_factors) if m.f_kind[f] == M.F_VECTOR]
    links = {u: [] for u in unaries}
    for k in range(m.n_messages):
        u, p, s = int(m.m_left[k]), int(m.m_right[k]), int(m.mtypes[int(m.m_type[k])].param)
        v = side_unary[(p, 1 - s)]
        assert v != u
        links[u].append((p, s, v))
    return unaries, links


def cost_line(m, coff, p, side, x_other):
    """cost_p(x, x_other) over x when the unary is on side 0, cost_p(x_other, x) when on side 1: the pairwise cost of
    include/lpmp_model.h (DENSE: the table entry; POTTS: a == b ? 0.0 : diff; SHARED / DIFF / DIFF_SHIFT: ONE multiply scale * entry)"""
    kind, d0, d1 = int(m.f_kind[p]), int(m.f_dim0[p]), int(m.f_dim1[p])
    c = int(coff[p])
    if kind == M.F_PAIRWISE_DENSE:
        T = m.const_data[c:c + d0 * d1].reshape(d0, d1)
        return T[:, x_other].copy() if side == 0 else T[x_other, :].copy()
    if kind == M.F_PAIRWISE_POTTS:
        line = np.full(d0, m.const_data[c], np.float64)
        line[x_other] = 0.0
        return line
    scale = m.const_data[c]
    t = int(m.f_table[p])
    if kind == M.F_PAIRWISE_SHARED:
        V = m.shared_table(t)
        return scale * (V[:, x_other] if side == 0 else V[x_other, :])
    if kind == M.F_PAIRWISE_DIFF_SHIFT:      # scale * D[clip(a - b + shift, 0, n - 1)], the shift converted as the device converts it
        n, s = int(m.sh_dim1[t]), M.diff_shift_int(m.const_data[c + 1])
        D = m.sh_data[int(m.sh_off[t]): int(m.sh_off[t]) + n]
        k = np.arange(d0) - x_other + s if side == 0 else x_other - np.arange(d1) + s
        return scale * D[np.clip(k, 0, n - 1)]
    assert kind == M.F_PAIRWISE_DIFF
    D = m.sh_data[int(m.sh_off[t]): int(m.sh_off[t]) + d0 + d1 - 1]
    if side == 0:
        return scale * D[np.arange(d0) - x_other + d1 - 1]
    return scale * D[x_other - np.arange(d1) + d1 - 1]


def decode_order(m, order):
    """pi: ``order`` (all factors, as Plan.order(direction) / Oracle.order(direction) give it) restricted to the VECTOR factors"""
    return [int(f) for f in order if m.f_kind[f] == M.F_VECTOR]


def decode_reference(m, duals, order, refine=0, sweeps_out=None):
    """The labels of lpmp_decode_primal as the [n_factors, 2] array lpmp_download_primal returns: vector factor (label, 0), pairwise
    factor (label of its side-0 unary, label of its side-1 unary).  ``duals``: the packed duals; ``order``: all factors in the
    order of the direction.  ``sweeps_out`` (a list): receives a copy of the array after the initial and after every refinement sweep."""
    duals = np.asarray(duals, np.float64)
    unaries, links = structure(m)
    doff, coff = m.dual_offsets(), m.const_offsets()
    pi = decode_order(m, order)
    assert sorted(pi) == unaries
    pos = {u: i for i, u in enumerate(pi)}
    label = {}

    def primal():
        out = np.zeros((m.n_factors, 2), np.int32)
        for u in unaries:
            out[u, 0] = label[u]
            for p, s, _ in links[u]:
                out[p, s] = label[u]
        return out

    for sweep in range(refine + 1):
        for u in pi:
            d0 = int(m.f_dim0[u])
            c = duals[doff[u]:doff[u] + d0].copy()
            for p, s, v in links[u]:
                if sweep == 0 and pos[v] > pos[u]:
                    continue
                t = cost_line(m, coff, p, s, label[v])
                ms = duals[doff[p] + (0 if s == 0 else int(m.f_dim0[p])):][:d0]
                c = c + (t + ms)
            label[u] = int(np.argmin(c))          # the first minimiser; all +inf: 0
        if sweeps_out is not None:
            sweeps_out.append(primal())
    return primal()


def level_reference(m, order):
    """(unaries in pi, levels): level(u) = 1 + max level(v) over the neighbours v earlier in pi, 1 without any"""
    _, links = structure(m)
    pi = decode_order(m, order)
    pos = {u: i for i, u in enumerate(pi)}
    level = {}
    for u in pi:
        level[u] = 1 + max([level[v] for _, _, v in links[u] if pos[v] < pos[u]], default=0)
    return np.asarray(pi, np.int32), np.asarray([level[u] for u in pi], np.int32)


def energy(m, primal):
    """the original energy of a labelling: ``m.dual_data`` holds the original unaries (and zero messages)"""
    _, links = structure(m)
    doff, coff = m.dual_offsets(), m.const_offsets()
    e = float(m.constant)
    for f in range(m.n_factors):
        if m.f_kind[f] == M.F_VECTOR:
            e += float(m.dual_data[doff[f] + primal[f, 0]])
        else:
            a, b = int(primal[f, 0]), int(primal[f, 1])
            e += float(cost_line(m, coff, f, 0, b)[a])
            assert np.all(m.dual_data[doff[f]:doff[f + 1]] == 0.0)
    return e


def brute_force(m):
    """the minimum of ``energy`` over all labellings (tiny models)"""
    unaries, links = structure(m)
    best = INF
    for labels in itertools.product(*[range(int(m.f_dim0[u])) for u in unaries]):
        lab = dict(zip(unaries, labels))
        pr = np.zeros((m.n_factors, 2), np.int32)
        for u in unaries:
            pr[u, 0] = lab[u]
            for p, s, _ in links[u]:
                pr[p, s] = lab[u]
        best = min(best, energy(m, pr))
    return best


# ---- models --------------------------------------------------------------------------------------------------------------------
def build_model(unaries, edges, msgs=None, mtypes=None):
    """A pairwise model over variables 0 .. n-1 in variable order.  ``unaries``: one cost vector per variable (any lengths);
    ``edges``: (i, j, spec) with variable i on side 0 and j on side 1 of the pairwise factor (i > j is allowed), spec one of
    ("dense", T [d_i, d_j]), ("potts", diff), ("shared", V [d_i, d_j], scale), ("diff", D [d_i + d_j - 1], scale) — arrays that are
    the same object share one pool entry.  ``msgs``: (message type, variable, edge) triples instead of the two messages per edge."""
    b = M.ModelBuilder(2, mtypes if mtypes is not None else S.mrf_mtypes())
    u = [int(b.add_vector_factors(0, np.asarray(c, np.float64)[None])[0]) for c in unaries]
    pool = {}

    def entry(a, vec):
        if id(a) not in pool:
            pool[id(a)] = b.add_diff_table(a) if vec else b.add_shared_table(a)
        return pool[id(a)]

    p = []
    for i, j, spec in edges:
        di, dj = len(unaries[i]), len(unaries[j])
        if spec[0] == "dense":
            T = np.asarray(spec[1], np.float64)
            assert T.shape == (di, dj)
            p.append(int(b.add_dense_pairwise(1, T)[0]))
        elif spec[0] == "potts":
            assert di == dj
            p.append(int(b.add_potts_pairwise(1, di, [spec[1]])[0]))
        elif spec[0] == "shared":
            assert spec[1].shape == (di, dj)
            p.append(int(b.add_shared_pairwise(1, [entry(spec[1], False)], [spec[2]])[0]))
        else:
            assert spec[0] == "diff" and spec[1].shape == (di + dj - 1,)
            p.append(int(b.add_diff_pairwise(1, di, dj, [entry(spec[1], True)], [spec[2]])[0]))
    if msgs is None:
        msgs = [x for e, (i, j, _) in enumerate(edges) for x in ((0, i, e), (1, j, e))]
    for t, v, e in msgs:
        b.add_messages(t, [u[v]], [p[e]])
    for e, (i, j, _) in enumerate(edges):
        lo, hi = min(i, j), max(i, j)
        b.add_relations([u[lo], p[e]], [p[e], u[hi]])
    return b.finish()


def _rng(seed):
    return np.random.default_rng(seed)


@functools.lru_cache(maxsize=None)
def grid(H, W, L, order, pairwise="dense", seed=5):
    return S.grid_model(H, W, L, pairwise=pairwise, order=order, seed=seed)


@functools.lru_cache(maxsize=None)
def random_graph(n=60, m=150, L=8, pairwise="dense", seed=3):
    return S.random_graph_model(n, m, L, seed=seed, pairwise=pairwise)


@functools.lru_cache(maxsize=None)
def star(n_leaves=70, L=5, seed=2):
    """a hub in the middle of the variable order with ``n_leaves`` neighbours, on alternating sides of its tables"""
    r = _rng(seed)
    hub = n_leaves // 2
    un = [r.random(L) for _ in range(n_leaves + 1)]
    leaves = [v for v in range(n_leaves + 1) if v != hub]
    edges = [((hub, v) if k % 2 else (v, hub)) + (("dense", r.random((L, L))),) for k, v in enumerate(leaves)]
    return build_model(un, edges)


@functools.lru_cache(maxsize=None)
def duplicate_edges(L=6, seed=4):
    """two pairwise factors between variables 0 and 1 (one of them the other way round), and a third variable"""
    r = _rng(seed)
    un = [r.random(L) for _ in range(3)]
    return build_model(un, [(0, 1, ("dense", r.random((L, L)))), (1, 0, ("dense", r.random((L, L)))), (1, 2, ("potts", 0.4)),
                            (0, 1, ("potts", 0.3))])


@functools.lru_cache(maxsize=None)
def chain(seed, n=6, L=3):
    """the chains of DESIGN.md 8: n variables, L labels, U(0, 1) costs"""
    r = _rng(seed)
    un = [r.random(L) for _ in range(n)]
    return build_model(un, [(i, i + 1, ("dense", r.random((L, L)))) for i in range(n - 1)])


@functools.lru_cache(maxsize=None)
def table_grid(kind, order, H=24, W=24, L=8):
    """the 24 x 24 grids of the table in DESIGN.md 8: np.random.default_rng(3), unaries U(0, 1), tables U(0, 1) ("random") or
    min(|a - b|, 2) * w_e with w_e ~ U(0.1, 0.5) ("truncated")"""
    r = _rng(3)
    a, bb = S.grid_edges(H, W)
    var = S.grid_variable_order(H, W, order).reshape(-1)
    i, j = np.minimum(var[a], var[bb]), np.maximum(var[a], var[bb])
    un = r.random((H * W, L))
    if kind == "random":
        T = r.random((i.shape[0], L, L))
    else:
        ab = np.minimum(np.abs(np.arange(L)[:, None] - np.arange(L)[None, :]), 2).astype(np.float64)
        T = ab[None] * r.uniform(0.1, 0.5, i.shape[0])[:, None, None]
    return S.mrf_model(H * W, L, i, j, un, tables=T)


def small_graph(L, seed, kind="dense", ints=False, inf=False):
    """five variables of L labels: a 4-cycle with a chord and a pendant variable (more than one level, degrees 1 to 3)"""
    r = _rng(seed)
    draw = (lambda *s: r.integers(0, 3, s).astype(np.float64)) if ints else (lambda *s: r.random(s))
    un = [draw(L) for _ in range(5)]
    pairs = [(0, 1), (1, 2), (3, 2), (0, 3), (0, 2), (4, 2)]
    V = draw(L, L)
    D = draw(2 * L - 1)
    edges = []
    for k, (i, j) in enumerate(pairs):
        if kind == "dense":
            T = draw(L, L)
            if inf:                                   # some +inf entries; every row and column keeps finite ones
                T[r.random((L, L)) < 0.3] = INF
                T[np.arange(L), np.arange(L)] = draw(L)
            spec = ("dense", T)
        elif kind == "potts":
            spec = ("potts", float(draw(1)[0]) + (1.0 if ints else 0.0))
        elif kind == "shared":
            spec = ("shared", V, 0.5 + k if ints else 0.5 + float(r.random()))
        else:
            spec = ("diff", D, 0.5 + k if ints else 0.5 + float(r.random()))
        edges.append((i, j, spec))
    return build_model(un, edges)


@functools.lru_cache(maxsize=None)
def labels_case(L, kind="dense"):
    return small_graph(L, 100 + L, kind)


@functools.lru_cache(maxsize=None)
def ties_case(kind):
    return small_graph(6, 7, kind, ints=True)


@functools.lru_cache(maxsize=None)
def inf_tables_case():
    return small_graph(7, 9, "dense", inf=True)


@functools.lru_cache(maxsize=None)
def f32_case(L=13):
    """dense tables whose entries are exactly floats (the strict "f32" table precision accepts them)"""
    r = _rng(21)
    un = [r.random(L) for _ in range(4)]
    f = lambda *s: r.random(s).astype(np.float32).astype(np.float64)
    return build_model(un, [(0, 1, ("dense", f(L, L))), (2, 1, ("dense", f(L, L))), (2, 3, ("dense", f(L, L))), (0, 3, ("dense", f(L, L)))])


@functools.lru_cache(maxsize=None)
def rect_case(d0, d1):
    """rectangular d0 x d1 tables with the middle variable on either side, and a square one"""
    r = _rng(d0 * 100 + d1)
    un = [r.random(d0), r.random(d1), r.random(d0), r.random(d1)]
    return build_model(un, [(0, 1, ("dense", r.random((d0, d1)))), (2, 1, ("dense", r.random((d0, d1)))), (2, 3, ("dense", r.random((d0, d1)))),
                            (3, 1, ("dense", r.random((d1, d1)))), (0, 2, ("dense", r.random((d0, d0))))])


@functools.lru_cache(maxsize=None)
def diff_case(banded, L=40):
    """DIFF factors over full (random) or banded (truncated linear) vectors, square and rectangular"""
    r = _rng(31 + banded)
    L2 = L - 7
    if banded:
        D, D2 = M.truncated_linear(L, L, 0.05, 0.2), M.truncated_linear(L, L2, 0.04, 0.16)
    else:
        D, D2 = r.random(2 * L - 1), r.random(L + L2 - 1)
    un = [r.random(L), r.random(L), r.random(L2), r.random(L)]
    return build_model(un, [(0, 1, ("diff", D, 0.7)), (1, 3, ("diff", D, 1.3)), (3, 0, ("diff", D, 0.9)), (1, 2, ("diff", D2, 1.1)), (0, 2, ("diff", D2, 0.6))])


@functools.lru_cache(maxsize=None)
def mixed_case():
    """one neighbourhood holding every kind: variable 3 (13 labels) between dense (either side, rectangular), Potts, SHARED, DIFF
    (full and banded) factors; an isolated variable and one whose costs are all +inf (its c is all +inf: label 0)"""
    r = _rng(41)
    dims = [9, 5, 13, 13, 7, 11, 13, 13, 4, 3]
    un = [r.random(d) for d in dims]
    un[9] = np.full(3, INF)
    V = r.random((13, 7))
    Dfull = r.random(13 + 11 - 1)
    Dband = M.truncated_linear(13, 13, 0.1, 0.2)
    edges = [(3, 0, ("dense", r.random((13, 9)))), (1, 3, ("dense", r.random((5, 13)))), (2, 3, ("potts", 0.35)), (3, 4, ("shared", V, 0.8)),
             (3, 5, ("diff", Dfull, 1.2)), (6, 3, ("diff", Dband, 0.9)), (3, 7, ("potts", 0.15)), (2, 6, ("dense", r.random((13, 13)))),
             (7, 4, ("shared", V, 1.4)), (0, 5, ("dense", r.random((9, 11))))]
    return build_model(un, edges)
