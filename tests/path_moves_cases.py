"""Path moves (lpmp_path_moves): the numpy statement of the rule and the models of tests/test_path_moves_host.py and
tests/test_path_moves_gpu.py.  Written from the rule as include/lpmp_engine.h states it, not from the device code.  Models are
built once per process and never modified."""
import functools
import itertools

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

from decode_cases import brute_force, build_model, cost_line, energy, structure, table_grid  # noqa: F401  (the tests take them from here)

INF = float("inf")


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def path_edges(path, links):
    """[(pairwise factor, side of u_i in it)] for the k - 1 path edges: the ONE pairwise factor between consecutive members"""
    out = []
    for a, b in zip(path[:-1], path[1:]):
        cand = [(p, s) for p, s, v in links[a] if v == b]
        assert len(cand) == 1, (a, b, cand)
        out.append(cand[0])
    return out


def relabel_path(m, duals, label, path, links, doff, coff):
    """one path: node costs, forward recursion, back-tracking; ``label`` (unary -> label, any integers) is updated in place"""
    k = len(path)
    edges = path_edges(path, links)
    n = []
    for i, u in enumerate(path):
        d = int(m.f_dim0[u])
        mine = {edges[j][0] for j in (i - 1, i) if 0 <= j < k - 1}
        c = duals[doff[u]:doff[u] + d].copy()
        for p, s, v in links[u]:                                   # ascending message index
            ms = duals[doff[p] + (0 if s == 0 else int(m.f_dim0[p])):][:d]
            if p in mine:
                c = c + ms
            else:
                xv = min(max(int(label[v]), 0), int(m.f_dim0[v]) - 1)
                c = c + (cost_line(m, coff, p, s, xv) + ms)
        n.append(c)
    f = n[0]
    back = []
    with np.errstate(invalid="ignore"):
        for i in range(1, k):
            p, s_prev = edges[i - 1]
            d = int(m.f_dim0[path[i]])
            # C[x, y] = cost_e(x, y) when u_{i-1} is on side 0 of the edge, cost_e(y, x) otherwise
            Cxy = np.stack([cost_line(m, coff, p, s_prev, y) for y in range(d)], axis=1)
            V = f[:, None] + Cxy
            b = np.argmin(V, axis=0)                               # the smallest minimising x; an all +inf column: 0
            back.append(b)
            f = V[b, np.arange(d)] + n[i]
    x = int(np.argmin(f))                                          # the smallest minimiser; all +inf: 0
    for i in range(k - 1, 0, -1):
        label[path[i]] = x
        x = int(back[i - 1][x])
    label[path[0]] = x


def propagate(m, primal, links):
    """primal_propagate_kernel: both slots of every pairwise factor take the labels of its unaries that hold one"""
    for u, lk in links.items():
        if primal[u, 0] < m.f_dim0[u]:
            for p, s, _ in lk:
                primal[p, s] = primal[u, 0]
    return primal


def path_moves_reference(m, duals, primal, groups, rounds=1, trace=None, per_path=None):
    """The labels after lpmp_path_moves as the [n_factors, 2] array lpmp_download_primal returns, from the array ``primal`` it
    starts on.  ``trace`` (a list): a copy of the array, propagated, after every group of every round.  ``per_path`` (a callable):
    called with the label dict after every path."""
    duals = np.asarray(duals, np.float64)
    unaries, links = structure(m)
    doff, coff = m.dual_offsets(), m.const_offsets()
    out = np.array(primal, np.int32, copy=True)
    label = {u: int(out[u, 0]) for u in unaries}
    for _ in range(rounds):
        for g in groups:
            for path in g:
                relabel_path(m, duals, label, [int(u) for u in path], links, doff, coff)
                if per_path is not None:
                    per_path(label)
            if trace is not None:
                t = out.copy()
                for u in unaries:
                    t[u, 0] = label[u]
                trace.append(propagate(m, t, links))
    if rounds > 0 and any(len(g) for g in groups):
        for u in unaries:
            out[u, 0] = label[u]
        propagate(m, out, links)
    return out


def labels_to_primal(m, labels):
    """[n_factors, 2] from {unary: label} (every unary labelled)"""
    unaries, links = structure(m)
    pr = np.zeros((m.n_factors, 2), np.int32)
    for u in unaries:
        pr[u, 0] = labels[u]
    return propagate(m, pr, links)


def random_primal(m, seed):
    unaries, _ = structure(m)
    r = np.random.default_rng(seed)
    return labels_to_primal(m, {u: int(r.integers(0, int(m.f_dim0[u]))) for u in unaries})


def best_over_path(m, primal, path):
    """exhaustive search: the minimum of ``energy`` over the labels of ``path`` with all other labels as in ``primal``"""
    unaries, links = structure(m)
    base = {u: int(primal[u, 0]) for u in unaries}
    best = INF
    for labels in itertools.product(*[range(int(m.f_dim0[u])) for u in path]):
        base.update(zip(path, labels))
        best = min(best, energy(m, labels_to_primal(m, base)))
    return best


# ---- models --------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def _spec(r, kind, di, dj, ints=False, pool=None):
    draw = (lambda *s: r.integers(0, 3, s).astype(np.float64)) if ints else (lambda *s: r.random(s))
    if kind == "dense":
        return ("dense", draw(di, dj))
    if kind == "dense_f32":
        return ("dense", r.random((di, dj)).astype(np.float32).astype(np.float64))
    if kind == "potts":
        assert di == dj
        return ("potts", float(draw(1)[0]) + (1.0 if ints else 0.0))
    key = (kind, di, dj)
    if kind == "shared":
        if key not in pool:
            pool[key] = draw(di, dj)
        return ("shared", pool[key], 1.0 + float(r.integers(0, 3)) if ints else 0.5 + float(r.random()))
    if kind == "diff":
        if key not in pool:
            pool[key] = draw(di + dj - 1)
        return ("diff", pool[key], 1.0 + float(r.integers(0, 3)) if ints else 0.5 + float(r.random()))
    assert kind == "diff_banded" and di == dj
    if key not in pool:
        pool[key] = M.truncated_linear(di, dj, 0.05, 0.2)
    return ("diff", pool[key], 0.5 + float(r.random()))


@functools.lru_cache(maxsize=None)
def ladder(dims, kind="dense", seed=1, ints=False, flip="alternate"):
    """Two rails of len(dims) variables (rail A: variables 0 .. k-1, rail B: k .. 2k-1, both with the label counts ``dims``) and a
    rung between A_i and B_i: each rail is a path with one off-path neighbour per member.  ``flip``: "alternate" puts the members
    on alternating sides of their path edges (edge i runs from A_{i+1} to A_i for odd i), "none" keeps the earlier member on side 0,
    "all" on side 1.  Returns (model, [[rail A], [rail B]] as two GROUPS of one path each)."""
    r = _rng(seed)
    k = len(dims)
    pool = {}
    un = [(r.integers(0, 3, d).astype(np.float64) if ints else r.random(d)) for d in tuple(dims) * 2]
    edges = []
    for base in (0, k):
        for i in range(k - 1):
            a, b = base + i, base + i + 1
            if flip == "all" or (flip == "alternate" and i % 2):
                a, b = b, a
            edges.append((a, b, _spec(r, kind, len(un[a]), len(un[b]), ints, pool)))
    for i in range(k):
        a, b = (i, k + i) if i % 2 == 0 else (k + i, i)
        edges.append((a, b, _spec(r, kind, len(un[a]), len(un[b]), ints, pool)))
    return build_model(un, edges), [[list(range(k))], [list(range(k, 2 * k))]]


@functools.lru_cache(maxsize=None)
def labels_case(L, kind="dense"):
    """a 3-rung ladder of L labels, members on alternating sides"""
    return ladder((L, L, L), kind, seed=200 + L)


@functools.lru_cache(maxsize=None)
def rect_case():
    """rectangular tables along one path — 5, 40, 9, 70 labels on rail A (the wave form's limit is 64) and 3, 300, 7, 257 on rail C
    (the back-pointers of a node behind one of more than 256 labels take two bytes) — both rails in ONE group, a third variable row
    B between them so that no pairwise factor joins the two paths"""
    r = _rng(77)
    dA, dB, dC = (5, 40, 9, 70), (4, 4, 4, 4), (3, 300, 7, 257)
    un = [r.random(d) for d in dA + dB + dC]
    edges = []
    for base, dims in ((0, dA), (4, dB), (8, dC)):
        for i in range(3):
            a, b = (base + i, base + i + 1) if i % 2 == 0 else (base + i + 1, base + i)
            edges.append((a, b, ("dense", r.random((len(un[a]), len(un[b]))))))
    for i in range(4):
        edges.append((i, 4 + i, ("dense", r.random((len(un[i]), 4)))))
        edges.append((8 + i, 4 + i, ("dense", r.random((len(un[8 + i]), 4)))))
    return build_model(un, edges), [[[0, 1, 2, 3], [8, 9, 10, 11]], [[4, 5, 6, 7]]]


@functools.lru_cache(maxsize=None)
def long_case(k=300, L=3):
    return ladder((L,) * k, "dense", seed=9)


@functools.lru_cache(maxsize=None)
def pair512_case():
    """a 2-node path of 512 x 512 (a DIFF factor: no table of 2 MB) with a dense off-path neighbour of 3 labels at either end"""
    r = _rng(512)
    D = r.random(1023)
    un = [r.random(512), r.random(512), r.random(3), r.random(3)]
    return build_model(un, [(1, 0, ("diff", D, 0.7)), (0, 2, ("dense", r.random((512, 3)))), (3, 1, ("dense", r.random((3, 512))))]), [[[0, 1]], [[2], [3]]]


@functools.lru_cache(maxsize=None)
def inf_case():
    """+inf table entries on the path edges, an all +inf column (every x to label 2 of variable 1), and off-path lines with +inf"""
    r = _rng(13)
    L = 6
    un = [r.random(L) for _ in range(6)]

    def T():
        t = r.random((L, L))
        t[r.random((L, L)) < 0.3] = INF
        t[np.arange(L), np.arange(L)] = r.random(L)
        return t

    T01 = T()
    T01[:, 2] = INF
    edges = [(0, 1, ("dense", T01)), (2, 1, ("dense", T())), (2, 3, ("dense", T())), (0, 4, ("dense", T())), (5, 2, ("dense", T())), (4, 5, ("dense", T()))]
    return build_model(un, edges), [[[0, 1, 2, 3]], [[4, 5]]]


@functools.lru_cache(maxsize=None)
def all_inf_case():
    """every label of the last member costs +inf: label 0 there, back-pointers 0"""
    r = _rng(14)
    un = [r.random(4), r.random(4), np.full(4, INF)]
    return build_model(un, [(0, 1, ("dense", r.random((4, 4)))), (1, 2, ("dense", r.random((4, 4))))]), [[[0, 1, 2]]]


@functools.lru_cache(maxsize=None)
def mixed_path_case():
    """decode_cases.mixed_case(): every kind around variable 3, as path edges and as off-path lines"""
    from decode_cases import mixed_case
    # edges of mixed_case: 3-0 dense, 1-3 dense, 2-3 potts, 3-4 shared, 3-5 diff, 6-3 diff banded, 3-7 potts, 2-6 dense, 7-4 shared, 0-5 dense
    return mixed_case(), [[[1, 3, 4]], [[7, 3, 0]], [[0, 3, 2]], [[5, 3, 6]], [[0, 5]], [[8], [9], [2, 6]], [[4, 7]]]


@functools.lru_cache(maxsize=None)
def diff_shift_case(L=20):
    """a ladder of DIFF_SHIFT factors with non-zero shifts (windows that differ from unary to unary)"""
    r = _rng(61)
    k = 4
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = [int(b.add_vector_factors(0, r.random(L)[None])[0]) for _ in range(2 * k)]
    t = b.add_diff_table(M.truncated_linear(L, L, 0.05, 0.3))
    t2 = b.add_diff_table(r.random(2 * L + 5))
    pairs = []
    for base in (0, k):
        for i in range(k - 1):
            pairs.append((base + i, base + i + 1) if i % 2 == 0 else (base + i + 1, base + i))
    pairs += [(i, k + i) for i in range(k)]
    shifts = [L - 1 + int(s) for s in r.integers(-4, 5, len(pairs))]
    for e, (i, j) in enumerate(pairs):
        p = int(b.add_diff_shift_pairwise(1, L, L, [t if e % 2 else t2], [0.5 + float(r.random())], [shifts[e]])[0])
        b.add_messages(0, [u[i]], [p]); b.add_messages(1, [u[j]], [p])
        b.add_relations([u[min(i, j)], p], [p, u[max(i, j)]])
    return b.finish(), [[list(range(k))], [list(range(k, 2 * k))]]


@functools.lru_cache(maxsize=None)
def grid(H, W, L, order, pairwise="dense", seed=5):
    return S.grid_model(H, W, L, pairwise=pairwise, order=order, seed=seed)
