"""Models whose DIFF_SHIFT factors reference vectors with constant tails (the banded form of the shifted kernel), used by
tests/test_diff_shift_band_host.py and tests/test_diff_shift_band_gpu.py, and the numpy statement of the banded receive.

The yardstick of every model is the CPU oracle on the dense expansion (``expand(m)``).  Whether a model's launches are expected on
the shifted banded kernel comes from ``model.diff_band`` and the rule (``banded(m)``), never from the planner.

A receive of a d0 x d1 DIFF_SHIFT factor sees D through E[i] = D[clip(i - off, 0, n - 1)], i = a - b + d1 - 1, off = d1 - 1 - s.
The PLACEMENTS below put the band [lo, hi] of D at named places of E's ne = d0 + d1 - 1 entries by choosing s."""
import dataclasses

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

import diff_band_cases as B
import diff_shift_cases as C

MODES = C.MODES
ORDERS = C.ORDERS
expand = C.expand
grid_shape = C.grid_shape
n_edges = C.n_edges
# the LDS size classes of the banded layout (label counts rounded up to 64) and its edge between four and two waves (320 | 321)
GRID_LABELS = (3, 40, 64, 65, 130, 320, 321, 512)
PLACEMENTS = ("centred", "clipped_left", "clipped_right", "wholly_left", "wholly_right", "zero", "plain", "far_minus", "far_plus",
              "huge_minus", "huge_plus")
RECT_CHAINS = (dict(n=9, seed=3, dims=(5, 9)), dict(n=8, seed=8, dims=(3, 27)), dict(n=6, seed=5, dims=(70, 33)))
RTYPES = (M.RTYPE_SHARED, M.RTYPE_RESIDUAL)


# ---- the numpy statement of a receive ----------------------------------------------------------------------------------------
def expanded_vector(D, d0, d1, shift):
    """E: the ne entries a d0 x d1 receive indexes by i = a - b + d1 - 1 (what expand_diff() writes into the dense table)"""
    D = np.asarray(D, np.float64)
    k = np.arange(d0 + d1 - 1) - (d1 - 1)
    return D[np.clip(k + M.diff_shift_int(shift), 0, D.size - 1)]


def minplus_expanded(D, d0, d1, scale, shift, mo, side):
    """q[x] = min_y (fl(scale * T[a, b]) + m_o[y]) over every pair of expand_diff()'s table T[a, b] = D[clip(a - b + s, 0, n - 1)]"""
    D = np.asarray(D, np.float64)
    a, b = np.arange(d0)[:, None], np.arange(d1)[None, :]
    with np.errstate(invalid="ignore"):
        T = np.float64(scale) * D[np.clip(a - b + M.diff_shift_int(shift), 0, D.size - 1)]
        return B._tmin_reduce(T + mo[None, :], 1) if side == 0 else B._tmin_reduce(T.T + mo[None, :], 1)


def minplus_shift_banded(D, d0, d1, scale, shift, mo, side):
    """the same from the window [le, he] = model.diff_shift_band and the two tail terms (sweep_diff_shift_band_kernel): window
    entries k = le ... he ascending, each scale * D[k - off] with no clamp, then cL + pre / cR + suf as diff_band_cases.minplus_banded"""
    D = np.asarray(D, np.float64)
    n, ne = D.size, d0 + d1 - 1
    le, he = M.diff_shift_band(D, d0, d1, shift)
    off = d1 - 1 - M.diff_shift_int(shift)
    own, oth = (d0, d1) if side == 0 else (d1, d0)
    with np.errstate(invalid="ignore"):
        cL, cR = np.float64(scale) * D[0], np.float64(scale) * D[n - 1]
        sB = np.float64(scale) * D[le - off: he - off + 1] if he >= le else np.zeros(0)      # (inside [lo, hi]: no clamp)
        assert sB.size == max(0, he - le + 1)
        k = B._k_index(d0, d1, side)
        inside = (k >= le) & (k <= he)
        t = np.where(inside, np.concatenate([sB, [0.0]])[np.where(inside, k - le, sB.size)] + mo[None, :], np.inf)
        q = B._tmin_reduce(t, 1)
        pre, suf = B._tmin_accumulate(mo), B._tmin_accumulate(mo[::-1])[::-1]
        x = np.arange(own)
        if side == 0:
            jp, js, cp, cs = x + d1 - 2 - he, x + d1 - le, cR, cL
        else:
            jp, js, cp, cs = le + x - d1, he + x - d1 + 2, cL, cR
        tp = cp + pre[np.clip(jp, 0, oth - 1)]
        ts = cs + suf[np.clip(js, 0, oth - 1)]
        q = np.where(jp >= 0, B._tmin(q, tp), q)
        q = np.where(js <= oth - 1, B._tmin(q, ts), q)
    assert ne > 0
    return q


# ---- vectors -------------------------------------------------------------------------------------------------------------------
def window_vector(n, lo, width, cL, cR, seed):
    """n entries: cL below lo, ``width`` random values in [0.05, 1) that differ from both tails, cR above"""
    D = np.empty(n)
    D[:lo] = cL
    D[lo + width:] = cR
    D[lo:lo + width] = np.random.default_rng(4000 + seed).uniform(0.05, 1.0, width)
    return D


def widest(d0, d1):
    """the widest band the rule admits for a d0 x d1 receive"""
    return (d0 + d1 - 1) // M.DIFF_BAND_DIV


def named_vectors(w, seed=0):
    """{name: D}, every band at most ``w`` entries wide (w >= 0): the vectors of the issue's case list"""
    V = {
        "n1": np.array([0.75]),
        "n2": np.array([0.25, 1.5]),
        "constant": np.full(7, 1.25),
        "empty_unequal": np.array([0.5, 2.0, 2.0, 2.0]),          # lo = 1, hi = 0: no window entry, and the tails differ
        "unequal": window_vector(w + 5, 2, w, 1.5, 2.25, seed),
        "equal": window_vector(w + 4, 3, w, 2.0, 2.0, seed + 1),
        "long": window_vector(3 * w + 40, w + 11, w, 1.75, 0.5, seed + 2),
        "zeros": np.concatenate([[-0.0, -0.0], np.random.default_rng(seed + 3).uniform(0.05, 1.0, w), [0.0, 0.0, 0.0]]),
    }
    if w >= 1:
        V["inf"] = window_vector(w + 6, 3, w, np.inf, np.inf, seed + 4)
    return V


def placement_shift(name, D, d0, d1):
    """the shift that puts the band of D at the named place of a d0 x d1 receive"""
    n, ne = int(np.asarray(D).size), d0 + d1 - 1
    lo, hi = M.diff_band(D)
    off = {"centred": (ne - 1) // 2 - (lo + hi) // 2,       # the middle of the band on the middle entry
           "clipped_left": -1 - lo,                            # E starts one entry inside the band (a band of one entry: just left of E)
           "clipped_right": ne - hi,                           # ... and ends one entry before the band does
           "wholly_left": -2 - hi,
           "wholly_right": ne + 1 - lo}.get(name)
    if off is not None:
        return d1 - 1 - off
    return {"zero": 0, "plain": d1 - 1, "far_minus": -(n + max(d0, d1)), "far_plus": n + max(d0, d1),
            "huge_minus": -M.DIFF_SHIFT_MAX, "huge_plus": M.DIFF_SHIFT_MAX}[name]


def feasible_shift(D, d0, d1, jitter=0):
    """+inf tails: a shift under which the entry of a == b (i = d1 - 1) is a band entry, so that every row and every column of the
    expansion keeps a finite entry — the middle of the band there, moved by ``jitter`` while it stays inside"""
    lo, hi = M.diff_band(D)
    mid = (lo + hi) // 2
    j = int(np.clip(mid + jitter, lo, hi))
    return j            # i - off = d1 - 1 - off = s: index s of D sits on the diagonal


def other_side_vectors(n, seed):
    return B.other_side_vectors(n, seed)


def receive_cases(dims=((7, 7), (5, 9), (9, 4), (11, 3))):
    """(name, D, d0, d1, shift) of the host test: every named vector at every placement, at square and rectangular dims, for the
    widest band the rule admits and for one entry"""
    for d0, d1 in dims:
        for w in sorted({1, widest(d0, d1)}):
            for vname, D in named_vectors(w, seed=d0 + d1).items():
                for p in PLACEMENTS:
                    yield "%s w%d %dx%d %s" % (vname, w, d0, d1, p), D, d0, d1, placement_shift(p, D, d0, d1)


# ---- models --------------------------------------------------------------------------------------------------------------------
def grid_vectors(L):
    """the vectors of label_grid(L): the named ones within the rule at L x L ([name], [D]); above 130 labels, where the grid has 17
    edges, the three with a window and the empty band"""
    w = widest(L, L)
    V = named_vectors(min(w, 5) if L <= 130 else w, seed=L)
    if L > 130:
        V = {k: V[k] for k in ("unequal", "empty_unequal", "long", "inf")}
    V["widest"] = window_vector(w + 3, 1, w, 1.0, 3.0, L + 9)
    if w < 1:
        V.pop("widest")
    return list(V), [V[k] for k in V]


def edge_shifts(names, vectors, L, E):
    """edge e uses vector e mod k at placement (e // k + 3 (e mod k)) mod len(PLACEMENTS): over the edges every vector meets most
    placements and every placement is met; a vector with +inf tails keeps its band on the diagonal (feasible_shift)"""
    k = len(vectors)
    s = np.zeros(E, np.int64)
    placed = []
    for e in range(E):
        t = e % k
        p = PLACEMENTS[(e // k + 3 * t) % len(PLACEMENTS)]
        if names[t] == "inf":
            s[e], p = feasible_shift(vectors[t], L, L, jitter=e // k % 3 - 1), "feasible"
        else:
            s[e] = placement_shift(p, vectors[t], L, L)
        placed.append((names[t], p))
    return s, placed


def label_grid(L, order, compute_primal=False, scales=None):
    H, W = grid_shape(L)
    names, V = grid_vectors(L)
    s, _ = edge_shifts(names, V, L, n_edges(H, W))
    return S.grid_model(H, W, L, pairwise="diff_shift", order=order, seed=L + 1, diff_tables=V, shifts=s, scales=scales, compute_primal=compute_primal)


def placements_of(L):
    H, W = grid_shape(L)
    names, V = grid_vectors(L)
    return edge_shifts(names, V, L, n_edges(H, W))[1]


def banded(m):
    """does the shifted rule admit EVERY receive of the model (model.diff_shift_is_banded for DIFF_SHIFT factors,
    model.diff_band_is_banded for plain DIFF ones: the numpy statement)?"""
    for f in np.flatnonzero((m.f_kind == M.F_PAIRWISE_DIFF_SHIFT) | (m.f_kind == M.F_PAIRWISE_DIFF)):
        D = m.shared_table(int(m.f_table[f])).reshape(-1)
        if not M.diff_shift_is_banded(D, int(m.f_dim0[f]), int(m.f_dim1[f])):
            return False
    return True


def rule_grid(L, extra, order="colour_major"):
    """both vectors with the widest band the rule admits at L x L (extra = 0) or one entry more (extra = 1)"""
    w = widest(L, L) + extra
    V = [window_vector(w + 9, 4, w, 2.0, 1.5, L + t) for t in range(2)]
    return C.shift_grid(7, 6, L, order=order, seed=L + 3, vectors=V)


def one_unbanded_grid(L=40, order="colour_major"):
    """a compact truncated-linear vector beside a random one, alternating over the edges: every launch references both"""
    V = [M.truncated_linear_compact(0.2, 0.6)[0], S.u01(2 * L - 1, 78)]
    return C.shift_grid(7, 6, L, order=order, seed=8, vectors=V)


def compact_grid(L=40, order="colour_major", trunc=(0.6, 0.9), seed=5, shifts=None):
    """compact truncated-linear vectors (a handful of entries whatever L), random shifts in [-(n + L), n + L]"""
    V = [M.truncated_linear_compact(0.2 + 0.1 * t, tr)[0] for t, tr in enumerate(trunc)]
    return C.shift_grid(7, 6, L, order=order, seed=seed, vectors=V, shifts=shifts)


def mixed_kinds_grid(L=24, H=6, W=5, order="colour_major", seed=4, diff_width=3):
    """a grid whose edges alternate between plain DIFF factors (a window of ``diff_width`` entries around a == b) and DIFF_SHIFT
    factors (a compact vector, random shifts): every record has peers of both kinds"""
    var = S.grid_variable_order(H, W, order).reshape(-1)
    a, bb = S.grid_edges(H, W)
    i, j = np.minimum(var[a], var[bb]), np.maximum(var[a], var[bb])
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = b.add_vector_factors(0, S.u01(H * W * L, seed).reshape(-1, L))
    lo_rel, hi_rel = B.centred(diff_width)
    td = b.add_diff_table(B.band_vector(L, L, lo_rel, hi_rel, 2.0, 1.5, seed=seed))
    Dc = M.truncated_linear_compact(0.25, 0.5)[0]
    ts = b.add_diff_table(Dc)
    rng = np.random.default_rng(seed)
    for e in range(len(a)):
        sc = float(rng.uniform(0.5, 2.0))
        if e % 2 == 0:
            p = int(b.add_diff_pairwise(1, L, L, [td], [sc])[0])
        else:
            p = int(b.add_diff_shift_pairwise(1, L, L, [ts], [sc], [int(rng.integers(-(Dc.size + L), Dc.size + L + 1))])[0])
        b.add_messages(0, u[i[e]], p); b.add_messages(1, u[j[e]], p)
        b.add_relations([u[i[e]], p], [p, u[j[e]]])
    return b.finish()


def rect_chain(n=9, seed=3, dims=(5, 9)):
    """diff_shift_cases.rect_chain on vectors within the rule of both shapes (da x db and db x da share ne), every placement"""
    rng = np.random.default_rng(seed)
    da, db = dims
    mt = [M.MsgType(0, 2, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(1, 2, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1),
          M.MsgType(1, 3, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(0, 3, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1)]
    b = M.ModelBuilder(4, mt)
    w = widest(da, db)
    V = [window_vector(w + 5, 2, w, 1.5, 2.25, seed), np.array([0.5, 2.0, 2.0, 2.0]), window_vector(3 * w + 20, w + 7, max(1, w // 2), 3.0, 1.25, seed + 1)]
    tab = [b.add_diff_table(v) for v in V]
    u = [int(b.add_vector_factors(i % 2, rng.uniform(0, 1, (1, da if i % 2 == 0 else db)))[0]) for i in range(n)]
    for i in range(n - 1):
        even = i % 2 == 0
        t = i % len(tab)
        d0, d1 = (da, db) if even else (db, da)
        s = placement_shift(PLACEMENTS[(i + 2 * t) % len(PLACEMENTS)], V[t], d0, d1)
        p = int(b.add_diff_shift_pairwise(2 if even else 3, d0, d1, [tab[t]], [rng.uniform(0.5, 2.0)], [s])[0])
        b.add_messages(0 if even else 2, u[i], p)
        b.add_messages(1 if even else 3, u[i + 1], p)
        b.add_relations([u[i], p], [p, u[i + 1]])
    return b.finish()


def with_shifts(m, seed):
    """the same model with another random shift in every DIFF_SHIFT factor"""
    rng = np.random.default_rng(seed)
    off = m.const_offsets()
    const = np.array(m.const_data, np.float64, copy=True)
    for f in np.flatnonzero(m.f_kind == M.F_PAIRWISE_DIFF_SHIFT):
        n = int(m.sh_dim1[m.f_table[f]])
        const[off[f] + 1] = float(rng.integers(-(n + 64), n + 65))
    return dataclasses.replace(m, const_data=const, _keep=[])


def with_pool(m, vectors):
    """the same model with the pool entries replaced (same lengths)"""
    data = m.sh_data.copy()
    for t, v in enumerate(vectors):
        v = np.asarray(v, np.float64)
        assert v.size == int(m.sh_dim1[t])
        data[int(m.sh_off[t]): int(m.sh_off[t]) + v.size] = v
    return dataclasses.replace(m, sh_data=data, _keep=[])


def repool_grid(L=40, order="colour_major"):
    """(model, banded pool, unbanded pool, another banded pool): vectors of 2 L - 1 entries, so that one length holds a band within
    the rule and a random vector beyond it"""
    n = 2 * L - 1
    w = widest(L, L)
    banded_a = [window_vector(n, 7, w, 2.0, 1.5, 1), window_vector(n, n - 9, 3, 0.5, 2.5, 2)]
    unbanded = [banded_a[0], S.u01(n, 91)]
    banded_b = [window_vector(n, 30, 2, 1.0, 1.0, 3), np.full(n, 0.75)]
    m = C.shift_grid(7, 6, L, order=order, seed=12, vectors=banded_a)
    return m, banded_a, unbanded, banded_b


def window_chain(seed=5, n_vars=8, full=200, win=64):
    """diff_shift_cases.window_case: a windowed chain on the compact truncated-linear vector, (model, centres)"""
    _, w, c = C.window_case(seed=seed, n_vars=n_vars, full=full, win=win)
    return w, c


def lower_bound_as_summed(flb, constant):
    """the total the engine forms from per-factor bounds (lpmp_lower_bound: blocks of the factor array, 256 partial sums striding a
    block, a halving tree over them, the blocks added to the constant in order) — so that a total can be compared bit for bit with
    the oracle's per-factor bounds although the oracle adds them in another order"""
    flb = np.asarray(flb, np.float64)
    nf = flb.size
    nb = min(1024, (nf + 255) // 256)
    per = (nf + nb - 1) // nb
    nb = (nf + per - 1) // per
    lb = np.float64(constant)
    for blk in range(nb):
        x = flb[blk * per: min(nf, (blk + 1) * per)]
        sh = np.zeros(256)
        for t in range(256):
            s = np.float64(0.0)
            for v in x[t::256]:
                s = s + v
            sh[t] = s
        w = 128
        while w >= 1:
            sh[:w] = sh[:w] + sh[w:2 * w]
            w //= 2
        lb = lb + sh[0]
    return float(lb)


def gpu_expansion_cases():
    """(name, model) of every model tests/test_diff_shift_band_gpu.py hands to the oracle as an expansion"""
    for L in GRID_LABELS:
        for order in ORDERS:
            yield "grid L%d %s" % (L, order), label_grid(L, order)
    for kw in RECT_CHAINS:
        yield "rect chain %r" % (kw,), rect_chain(**kw)
    yield "mixed kinds", mixed_kinds_grid()
    yield "compact", compact_grid()
    yield "one unbanded", one_unbanded_grid()
    for extra in (0, 1):
        yield "rule +%d" % extra, rule_grid(40, extra)
    yield "repool", repool_grid()[0]
    yield "window chain", window_chain()[0]
