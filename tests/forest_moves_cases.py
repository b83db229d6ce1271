"""Forest moves (lpmp_forest_moves): the numpy statement of the rule and the models of tests/test_forest_moves_host.py
and tests/test_forest_moves_gpu.py.  Written from the rule as include/lpmp_engine.h states it, on the pairwise kinds themselves
(decode_cases.cost_line), not from the device code.  Models are built once per process and never modified."""
import functools

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

from decode_cases import brute_force, build_model, cost_line, energy, structure  # noqa: F401  (the tests take them from here)
from path_moves_cases import _spec, labels_to_primal, propagate, random_primal  # noqa: F401

INF = float("inf")


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def _first(a, axis=None):
    return np.argmin(a, axis=axis)


def _last(a, axis=None):
    """the LARGEST minimiser (the variant the tie tests tell from the rule)"""
    a = np.asarray(a)
    if axis is None:
        return a.shape[0] - 1 - np.argmin(a[::-1])
    assert axis == 0
    return a.shape[0] - 1 - np.argmin(a[::-1], axis=0)


def relabel_forest(m, duals, label, un, par, links, doff, coff, variant=None):
    """one group: node costs on the labels the group starts on, the up sweep children before parents, the down sweep; ``label``
    (unary -> label, any integers) is updated in place.  ``variant="last"`` takes the largest minimiser everywhere."""
    argmin = _last if variant == "last" else _first
    un, par = [int(u) for u in un], [int(q) for q in par]
    parent = dict(zip(un, par))
    assert len(parent) == len(un)
    dim = lambda v: int(m.f_dim0[v])
    edge, children, n = {}, {v: [] for v in un}, {}
    for v in un:
        c = duals[doff[v]:doff[v] + dim(v)].copy()
        for p, s, w in links[v]:                                   # ascending message index
            ms = duals[doff[p] + (0 if s == 0 else int(m.f_dim0[p])):][:dim(v)]
            if w in parent:                                        # a member: a tree edge, to the parent or to a child
                if parent[v] == w:
                    assert v not in edge, (v, w)
                    edge[v] = (p, s)
                else:
                    assert parent[w] == v, "the members of a group must induce a forest: %d - %d" % (v, w)
                    children[v].append(w)
                c = c + ms
            else:
                xw = min(max(int(label[w]), 0), dim(w) - 1)
                c = c + (cost_line(m, coff, p, s, xw) + ms)
        n[v] = c
    depth = {}
    for v in un:
        walk = []
        while v not in depth and v != -1:
            walk.append(v)
            v = parent[v]
        d = depth[v] if v != -1 else -1
        for w in reversed(walk):
            d += 1
            depth[w] = d
    order = sorted(un, key=lambda v: -depth[v])                    # children before parents (stable: the order inside a level is free)
    f, g, back = {}, {}, {}
    with np.errstate(invalid="ignore"):
        for v in order:
            fv = n[v]
            for c in children[v]:
                assert len(set(children[v])) == len(children[v])
                fv = fv + g[c]
            f[v] = fv
            q = parent[v]
            if q == -1:
                continue
            p, s = edge[v]
            # C[x, y] = cost_e(x, y) when v is on side 0 of the edge, cost_e(y, x) otherwise
            Cxy = np.stack([cost_line(m, coff, p, s, y) for y in range(dim(q))], axis=1)
            V = fv[:, None] + Cxy
            b = argmin(V, axis=0)                                  # the smallest minimising x; an all +inf column: 0
            back[v] = b
            g[v] = V[b, np.arange(dim(q))]
    for v in reversed(order):                                      # parents before children
        q = parent[v]
        label[v] = int(argmin(f[v])) if q == -1 else int(back[v][label[q]])


def forest_moves_reference(m, duals, primal, groups, rounds=1, trace=None, variant=None):
    """The labels after lpmp_forest_moves as the [n_factors, 2] array lpmp_download_primal returns, from the array ``primal`` it
    starts on.  ``groups``: (unaries, parent) pairs.  ``trace`` (a list): a copy of the array, propagated, after every group of
    every round."""
    duals = np.asarray(duals, np.float64)
    unaries, links = structure(m)
    doff, coff = m.dual_offsets(), m.const_offsets()
    out = np.array(primal, np.int32, copy=True)
    label = {u: int(out[u, 0]) for u in unaries}
    for _ in range(rounds):
        for un, par in groups:
            relabel_forest(m, duals, label, un, par, links, doff, coff, variant)
            if trace is not None:
                t = out.copy()
                for u in unaries:
                    t[u, 0] = label[u]
                trace.append(propagate(m, t, links))
    if rounds > 0 and any(len(un) for un, _ in groups):
        for u in unaries:
            out[u, 0] = label[u]
        propagate(m, out, links)
    return out


def as_paths(groups):
    """forest groups whose trees are paths (parent = next member) back as the path groups of Engine.path_set"""
    out = []
    for un, par in groups:
        paths, cur = [], []
        for u, q in zip(un, par):
            cur.append(int(u))
            if q == -1:
                paths.append(cur)
                cur = []
        assert not cur
        out.append(paths)
    return out


def tree_stats(un, par):
    """(heights, diameters) of the trees of one group, recomputed from the parents alone: per root its height and the longest
    path (in edges) of its tree"""
    un, par = [int(u) for u in un], [int(q) for q in par]
    kids = {u: [] for u in un}
    for u, q in zip(un, par):
        if q != -1:
            kids[q].append(u)

    def down(v):                   # (height of v, diameter of v's subtree), without recursion limits on long chains
        stack, post = [v], []
        while stack:
            x = stack.pop()
            post.append(x)
            stack.extend(kids[x])
        h, d = {}, {}
        for x in reversed(post):
            hs = sorted([h[c] + 1 for c in kids[x]], reverse=True) + [0, 0]
            h[x] = hs[0]
            d[x] = max([hs[0] + hs[1]] + [d[c] for c in kids[x]])
        return h[v], d[v]

    roots = [u for u, q in zip(un, par) if q == -1]
    st = [down(r) for r in roots]
    return [s[0] for s in st], [s[1] for s in st]


# ---- models --------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


TREE7 = (-1, 0, 0, 1, 1, 1, 2)      # a root with two children, one of them with three children (and the other with one)


@functools.lru_cache(maxsize=None)
def tree_model(parents=TREE7, dims=None, kind="dense", seed=1, ints=False, sides="mixed", off_dim=None):
    """Variables 0 .. k-1 form the tree ``parents`` (variable index of the parent, -1 for the root); variable k + i is an off-tree
    neighbour of variable i (``off_dim`` labels, None: as many as variable i; joined by a dense table, or by ``kind`` where that
    kind takes the shape).  ``sides``: "child0" puts every child on side 0 of its tree edge, "child1" on side 1, "mixed"
    alternates.  ``kind`` may be a tuple of kinds, taken edge by edge.  Returns (model, [the tree as one group, the off-tree
    neighbours as a group of single nodes])."""
    r = _rng(seed)
    k = len(parents)
    dims = tuple(dims) if dims is not None else (5,) * k
    od = [dims[i] if off_dim is None else off_dim for i in range(k)]
    pool = {}
    draw = (lambda d: r.integers(0, 3, d).astype(np.float64)) if ints else (lambda d: r.random(d))
    un = [draw(d) for d in dims] + [draw(d) for d in od]
    kinds = (kind,) if isinstance(kind, str) else tuple(kind)
    edges = []
    for i in range(1, k):
        a, b = i, parents[i]
        if sides == "child1" or (sides == "mixed" and i % 2):
            a, b = b, a
        edges.append((a, b, _spec(r, kinds[(i - 1) % len(kinds)], len(un[a]), len(un[b]), ints, pool)))
    for i in range(k):
        a, b = (i, k + i) if i % 2 == 0 else (k + i, i)
        kd = kinds[i % len(kinds)]
        if len(un[a]) != len(un[b]) and kd in ("potts", "diff_banded"):
            kd = "dense"
        edges.append((a, b, _spec(r, kd, len(un[a]), len(un[b]), ints, pool)))
    tree = (np.arange(k, dtype=np.int32), np.asarray(parents, np.int32))
    off = (np.arange(k, 2 * k, dtype=np.int32), np.full(k, -1, np.int32))
    return build_model(un, edges), [tree, off]


@functools.lru_cache(maxsize=None)
def labels_case(L):
    """four nodes of L labels (a root, two children, a grandchild) with an off-tree neighbour of 3 labels each; 512: DIFF edges"""
    return tree_model((-1, 0, 0, 1), (L,) * 4, "dense" if L < 512 else "diff", seed=300 + L, off_dim=3)


@functools.lru_cache(maxsize=None)
def rect_case():
    """rectangular tree edges that put the wave form and the workgroup form at one height, and both back-pointer widths in one
    tree: root 0 (9 labels) <- 1 (300) <- 2 (40);  0 <- 3 (5) <- 4 (7);  3 <- 5 (257)"""
    return tree_model((-1, 0, 1, 0, 3, 3), (9, 300, 40, 5, 7, 257), "dense", seed=78, off_dim=4)


@functools.lru_cache(maxsize=None)
def fan_case(n_children):
    """a root with ``n_children`` children (more than 8: the child rows no longer fit a cache line of offsets)"""
    return tree_model((-1,) + (0,) * n_children, (6,) + (4,) * n_children, "dense", seed=400 + n_children, off_dim=3)


@functools.lru_cache(maxsize=None)
def diff_shift_tree(L=20):
    """TREE7 over DIFF_SHIFT factors with non-zero shifts, an off-tree neighbour per node"""
    r = _rng(62)
    k = len(TREE7)
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = [int(b.add_vector_factors(0, r.random(L)[None])[0]) for _ in range(2 * k)]
    t = b.add_diff_table(M.truncated_linear(L, L, 0.05, 0.3))
    t2 = b.add_diff_table(r.random(2 * L + 5))
    pairs = [((i, TREE7[i]) if i % 2 else (TREE7[i], i)) for i in range(1, k)] + [(i, k + i) for i in range(k)]
    shifts = [L - 1 + int(s) for s in r.integers(-4, 5, len(pairs))]
    for e, (i, j) in enumerate(pairs):
        p = int(b.add_diff_shift_pairwise(1, L, L, [t if e % 2 else t2], [0.5 + float(r.random())], [shifts[e]])[0])
        b.add_messages(0, [u[i]], [p]); b.add_messages(1, [u[j]], [p])
        b.add_relations([u[min(i, j)], p], [p, u[max(i, j)]])
    return b.finish(), [(np.arange(k, dtype=np.int32), np.asarray(TREE7, np.int32)), (np.arange(k, 2 * k, dtype=np.int32), np.full(k, -1, np.int32))]


@functools.lru_cache(maxsize=None)
def random_tree(seed):
    """a tree-structured MODEL of 4 to 7 unaries with 2 or 3 labels: node 0 has three children, child 1 on side 0 and child 2 on
    side 1 of its edge; the rest hangs on at random.  Returns (model, parents)"""
    r = _rng(1000 + seed)
    k = int(r.integers(4, 8))
    parents = [-1, 0, 0, 0] + [int(r.integers(0, i)) for i in range(4, k)]
    un = [r.random(int(r.integers(2, 4))) for _ in range(k)]
    edges = []
    for i in range(1, k):
        a, b = (i, parents[i]) if (i == 1 or (i > 2 and r.random() < 0.5)) else (parents[i], i)
        edges.append((a, b, ("dense", r.random((len(un[a]), len(un[b]))))))
    return build_model(un, edges), parents


@functools.lru_cache(maxsize=None)
def tiny_tree(seed):
    """tree models of 2 and 3 unaries (the sizes random_tree does not reach)"""
    r = _rng(2000 + seed)
    k = 2 + seed % 2
    parents = [-1, 0, 1][:k]
    un = [r.random(int(r.integers(2, 4))) for _ in range(k)]
    edges = []
    for i in range(1, k):
        a, b = (i, parents[i]) if i % 2 else (parents[i], i)
        edges.append((a, b, ("dense", r.random((len(un[a]), len(un[b]))))))
    return build_model(un, edges), parents


@functools.lru_cache(maxsize=None)
def thinned_grid(H=8, W=7, L=4, seed=11):
    """a grid with a third of its edges removed, every fifth remaining edge doubled (parallel pairwise factors) and the unaries
    that lost all their edges left isolated, plus two unaries that never had any"""
    r = _rng(seed)
    a, b = S.grid_edges(H, W)
    keep = r.random(a.shape[0]) > 1 / 3
    keep[[k for k in range(a.shape[0]) if a[k] == 0 or b[k] == 0]] = False         # variable 0: isolated
    n = H * W + 2
    un = [r.random(L) for _ in range(n)]
    edges = []
    for k in np.flatnonzero(keep):
        i, j = (int(a[k]), int(b[k])) if k % 2 else (int(b[k]), int(a[k]))
        edges.append((i, j, ("dense", r.random((L, L)))))
        if len(edges) % 5 == 0:
            edges.append((j, i, ("dense", r.random((L, L)))))
    return build_model(un, edges)


def whole_tree_group(m, parents):
    return [(np.arange(len(parents), dtype=np.int32), np.asarray(parents, np.int32))]


def graph_degree(m):
    _, links = structure(m)
    return max([len(l) for l in links.values()], default=0)
