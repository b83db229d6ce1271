"""Models whose difference vectors have constant tails (the banded form of class ``diff``), used by tests/test_diff_band_host.py
and tests/test_diff_band_gpu.py, and the numpy statement of the two reductions the device runs.

The yardstick of every model is the CPU oracle on the dense expansion (``expand(m)``), as in tests/diff_tables_cases.py: the host
test runs the oracle over every expansion listed here, the GPU test compares the engine on the DIFF model with it.  Whether a model's
launches are expected on the banded kernel comes from ``model.diff_band`` and the rule (``banded(m)``), never from the planner."""
import dataclasses
import functools

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

import diff_tables_cases as T

MODES = T.MODES
ORDERS = T.ORDERS
expand = T.expand
grid_shape = T.grid_shape

# every NI variant of the window loop (1 ... 4 own labels per lane), the second 256-label chunk, every LDS size, the scan carry
GRID_LABELS = (8, 33, 64, 65, 128, 130, 200, 257, 330, 449, 512)
HALF_WIDTHS = (0, 1, 2)          # (8 labels, half-width 2: 5 of 15 entries, beyond the rule — that grid runs the full kernel)
RULE_LABELS = (64, 130)          # the widest window the rule admits, and one entry wider
ASYM_LABELS = (37, 100)
ASYM_KINDS = ("left3", "offdiag", "unequal", "inf", "oneside", "constant")
SCALE_KINDS = ("one", "random", "negative", "zero")
RECT_CHAINS = (dict(n=9, seed=3, dims=(5, 9)), dict(n=12, seed=8, dims=(3, 27)), dict(n=7, seed=5, dims=(70, 33)), dict(n=5, seed=6, dims=(40, 200)))
RECT_WIDTHS = (1, 2, 3)
TIE_LABELS = (33, 130)
PRIMAL_LABELS = (16, 130)
RTYPES = T.RTYPES
MID_SIZE = (128, 128, 64)
N_FUZZ = 100


# ---- the numpy statement of a receive ----------------------------------------------------------------------------------------
def _tmin_reduce(t, axis):
    """minimum along an axis in the total order of the device's fmin: -0.0 below +0.0 (np.minimum leaves the sign of a tie open)"""
    q = np.minimum.reduce(t, axis=axis)
    neg0 = np.any((t == 0) & np.signbit(t), axis=axis)
    return np.where(q == 0, np.where(neg0, -0.0, 0.0), q)


def _tmin(a, b):
    return _tmin_reduce(np.stack(np.broadcast_arrays(a, b)), 0)


def _tmin_accumulate(v):
    """prefix minima in the same order"""
    q = np.minimum.accumulate(v)
    neg0 = np.logical_or.accumulate((v == 0) & np.signbit(v))
    return np.where(q == 0, np.where(neg0, -0.0, 0.0), q)


def _k_index(d0, d1, side):
    """k[x, y] = index into D of own label x against the other side's y"""
    own, oth = (d0, d1) if side == 0 else (d1, d0)
    x, y = np.arange(own)[:, None], np.arange(oth)[None, :]
    return (x - y if side == 0 else y - x) + d1 - 1


def minplus_full(D, d0, d1, scale, mo, side):
    """q[x] = min_y (fl(scale * D[k(x, y)]) + m_o[y]): every pair, what sweep_diff_kernel and the expansion compute"""
    with np.errstate(invalid="ignore"):
        sD = np.float64(scale) * np.asarray(D, np.float64)
        return _tmin_reduce(sD[_k_index(d0, d1, side)] + mo[None, :], 1)


def minplus_banded(D, d0, d1, scale, mo, side):
    """the same from the window [lo, hi] and the two tail terms (sweep_diff_band_kernel): window entries, then c + pre, then c + suf"""
    D = np.asarray(D, np.float64)
    n = d0 + d1 - 1
    lo, hi = M.diff_band(D)
    own, oth = (d0, d1) if side == 0 else (d1, d0)
    with np.errstate(invalid="ignore"):
        sD = np.float64(scale) * D
        cL, cR = np.float64(scale) * D[0], np.float64(scale) * D[n - 1]
        k = _k_index(d0, d1, side)
        t = np.where((k >= lo) & (k <= hi), sD[np.clip(k, 0, n - 1)] + mo[None, :], np.inf)
        q = _tmin_reduce(t, 1)
        pre, suf = _tmin_accumulate(mo), _tmin_accumulate(mo[::-1])[::-1]
        x = np.arange(own)
        if side == 0:
            jp, js, cp, cs = x + d1 - 2 - hi, x + d1 - lo, cR, cL
        else:
            jp, js, cp, cs = lo + x - d1, hi + x - d1 + 2, cL, cR
        tp = cp + pre[np.clip(jp, 0, oth - 1)]
        ts = cs + suf[np.clip(js, 0, oth - 1)]
        q = np.where(jp >= 0, _tmin(q, tp), q)
        q = np.where(js <= oth - 1, _tmin(q, ts), q)
    return q


def other_side_vectors(n, seed):
    """m_o of a receive: random, quantised with ties, with zeros of both signs, with +inf entries (never all of them)"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, n)
    b = rng.integers(0, 3, n).astype(np.float64)
    c = rng.integers(-1, 2, n).astype(np.float64)
    c[rng.uniform(size=n) < 0.5] *= -1.0                 # -0.0 where the entry was 0
    d = rng.uniform(-1, 1, n)
    d[rng.uniform(size=n) < 0.3] = np.inf
    d[int(rng.integers(n))] = 0.25
    return a, b, c, d


# ---- vectors -------------------------------------------------------------------------------------------------------------------
def band_vector(d0, d1, lo_rel, hi_rel, cL=2.0, cR=2.0, seed=0, integer=False):
    """D with the band [c + lo_rel, c + hi_rel] (c = d1 - 1, the entry of a == b), clipped to the vector: cL below it, cR above,
    inside it random values in [0.05, 1) — or integers in {0, 1} — that differ from both tails"""
    n = d0 + d1 - 1
    c = d1 - 1
    lo, hi = max(0, c + lo_rel), min(n - 1, c + hi_rel)
    rng = np.random.default_rng(1000 + seed)
    D = np.empty(n)
    D[:lo] = cL
    D[hi + 1:] = cR
    w = max(0, hi - lo + 1)
    D[lo:hi + 1] = rng.integers(0, 2, w).astype(np.float64) if integer else rng.uniform(0.05, 1.0, w)
    return D


def centred(width):
    """(lo_rel, hi_rel) of a window of ``width`` entries around a == b"""
    lo = -((width - 1) // 2)
    return lo, lo + width - 1


def widest(L):
    """the widest window the rule admits for an L x L factor"""
    return (2 * L - 1) // M.DIFF_BAND_DIV


def banded(m):
    """does the rule admit EVERY vector a DIFF factor of the model references (model.diff_band: the numpy statement)?"""
    ts = sorted({int(t) for t in m.f_table[m.f_kind == M.F_PAIRWISE_DIFF]})
    return all(M.diff_band_is_banded(m.shared_table(t).reshape(-1)) for t in ts)


def _scales(kind, E, seed):
    sc = 0.5 + 1.5 * S.u01(E, seed + 77)
    if kind == "one":
        return np.ones(E)
    if kind == "negative":
        sc[E // 2] = -0.75
    elif kind == "zero":
        sc[E // 3] = 0.0
    elif kind != "random":
        raise ValueError(kind)
    return sc


def band_grid(L, order, windows, tails=((2.0, 2.0), (1.5, 1.5)), scales="random", seed=None, shape=None, compute_primal=False,
              unaries=None, integer=False, n_scales=None):
    """grid whose vectors are band_vector(L, L, *windows[t], *tails[t]); ``n_scales``: the edges cycle through that many scales"""
    H, W = shape or grid_shape(L)
    E = H * (W - 1) + (H - 1) * W
    seed = L if seed is None else seed
    D = np.stack([band_vector(L, L, w[0], w[1], tl[0], tl[1], seed=seed + 13 * t, integer=integer) for t, (w, tl) in enumerate(zip(windows, tails))])
    sc = _scales(scales, E, seed)
    if n_scales:
        sc = sc[np.arange(E) % n_scales]
    return S.grid_model(H, W, L, pairwise="diff", order=order, seed=seed, n_tables=len(windows), diff_tables=D, scales=sc,
                        compute_primal=compute_primal, unaries=unaries)


def label_grid(L, order, r):
    """two vectors of half-width r: a window of random values, and a truncated linear potential min(slope |a - b|, slope (r + 1))"""
    H, W = grid_shape(L)
    E = H * (W - 1) + (H - 1) * W
    D = np.stack([band_vector(L, L, -r, r, 2.0, 2.0, seed=L + r), M.truncated_linear(L, L, 0.25, 0.25 * (r + 1))])
    sc = _scales("random", E, L)
    if L > 130:                                        # (four scales over the 17 edges: the numpy statement runs every (vector, scale))
        sc = sc[np.arange(E) % 4]
    return S.grid_model(H, W, L, pairwise="diff", order=order, seed=L, n_tables=2, diff_tables=D, scales=sc)


def rule_grid(L, order, extra):
    """the widest admitted window (extra = 0) or one entry more (extra = 1), in both vectors"""
    w = centred(widest(L) + extra)
    return band_grid(L, order, (w, w), seed=L + 3)


def truncated_grid(potential, L, trunc_labels, order="colour_major"):
    if potential == "linear":
        D = np.stack([M.truncated_linear(L, L, 0.1 + 0.05 * t, (0.1 + 0.05 * t) * trunc_labels) for t in range(2)])
    else:
        D = np.stack([M.truncated_quadratic(L, L, 0.01 + 0.003 * t, (0.01 + 0.003 * t) * (trunc_labels * trunc_labels)) for t in range(2)])
    return S.grid_model(7, 6, L, pairwise="diff", order=order, seed=14, n_tables=2, diff_tables=D)


def asym_vector(kind, L, t):
    n, c = 2 * L - 1, L - 1
    if kind == "left3":
        return band_vector(L, L, -3, 0, 2.0, 2.0, seed=t)
    if kind == "offdiag":                              # a - b in [5, 8]: no window entry for the first own labels of one side, the last of the other
        return band_vector(L, L, 5, 8, 1.25, 1.25, seed=t)
    if kind == "unequal":
        return band_vector(L, L, -2 - t, 1, 1.5, 2.25, seed=t)
    if kind == "inf":                                  # a window constraint: +inf outside |a - b| <= 1 + t (the diagonal keeps every row and column feasible)
        return band_vector(L, L, -1 - t, 1 + t, np.inf, np.inf, seed=t)
    if kind == "oneside":                              # a left tail only, the window reaching the last entry; a right tail only
        return band_vector(L, L, -c, -c + 3 + t, 0.0, 0.0, seed=t) if t else band_vector(L, L, c - 4, c, 1.75, 0.0, seed=t)
    if kind == "constant":
        return np.full(n, 0.5 + t)
    raise ValueError(kind)


def asym_grid(kind, L, order, scales):
    H, W = grid_shape(L)
    E = H * (W - 1) + (H - 1) * W
    D = np.stack([asym_vector(kind, L, t) for t in range(2)])
    return S.grid_model(H, W, L, pairwise="diff", order=order, seed=L + 1, n_tables=2, diff_tables=D, scales=_scales(scales, E, L))


def asym_scale_kinds(kind):
    return ("one", "random") if kind == "inf" else SCALE_KINDS       # +inf tails: positive scales only


def rect_chain(width, n=9, seed=3, dims=(5, 9)):
    """diff_tables_cases.rect_chain with windows of ``width`` entries: around a == b in the da x db vector, off it in the db x da one"""
    rng = np.random.default_rng(seed)
    da, db = dims
    mt = [M.MsgType(0, 2, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(1, 2, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1),
          M.MsgType(1, 3, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(0, 3, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1)]
    b = M.ModelBuilder(4, mt)
    w = centred(width)
    tab = [b.add_diff_table(band_vector(da, db, w[0], w[1], 1.5, 2.5, seed=seed)),
           b.add_diff_table(band_vector(db, da, 1, width, 3.0, 1.25, seed=seed + 1))]
    u = [int(b.add_vector_factors(i % 2, rng.uniform(0, 1, (1, da if i % 2 == 0 else db)))[0]) for i in range(n)]
    for i in range(n - 1):
        even = i % 2 == 0
        p = int(b.add_diff_pairwise(2 if even else 3, da if even else db, db if even else da, [tab[0 if even else 1]], [rng.uniform(0.5, 2.0)])[0])
        b.add_messages(0 if even else 2, u[i], p)
        b.add_messages(1 if even else 3, u[i + 1], p)
        b.add_relations([u[i], p], [p, u[i + 1]])
    return b.finish()


def ties_grid(L, order):
    """integer unaries in {0, 1, 2}, integer D (a 0 / 1 window, tails 2 and 1), scale 1: ties everywhere, exact sums"""
    H, W = grid_shape(L)
    un = np.floor(3.0 * S.u01(H * W * L, L + 5))
    return band_grid(L, order, ((-1, 1), (-2, 0)), tails=((2.0, 2.0), (2.0, 1.0)), scales="one", unaries=un, integer=True)


def primal_grid(L, order):
    return band_grid(L, order, ((-1, 1), (-2, 2)), seed=2, shape=(6, 5), compute_primal=True)


def rules_grid(H, W, L, order="row_major", seed=1, flags=0, blocks=0, sched=M.SCHED_LEFT):
    """diff_tables_cases.rules_grid with windows of half-width 1"""
    var = S.grid_variable_order(H, W, order).reshape(-1)
    a, bb = S.grid_edges(H, W)
    i, j = np.minimum(var[a], var[bb]), np.maximum(var[a], var[bb])
    mts = [M.MsgType(0, 1, sched, 0, 1, M.M_UNARY_PAIRWISE, 0, flags), M.MsgType(0, 1, sched, 0, 1, M.M_UNARY_PAIRWISE, 1, flags)]
    b = M.ModelBuilder(2, mts, None)
    u = b.add_vector_factors(0, S.u01(H * W * L, seed).reshape(-1, L))
    t = [b.add_diff_table(band_vector(L, L, -1, 1, 2.0 + q, 2.0 + q, seed=seed + q)) for q in range(2)]
    p = b.add_diff_pairwise(1, L, L, np.asarray(t)[np.arange(len(a)) % 2], 0.5 + 1.5 * S.u01(len(a), seed + 2))
    b.add_interleaved_messages(np.tile(np.array([0, 1], np.int32), len(a)), np.stack([u[i], u[j]], 1).reshape(-1), np.repeat(p, 2))
    b.add_relations(np.stack([u[i], p], 1).reshape(-1), np.stack([p, u[j]], 1).reshape(-1))
    if blocks:
        band = (np.arange(H * W) % W) * blocks // W
        for k in range(len(a)):
            if band[a[k]] == band[bb[k]]:
                b.put_in_same_partition(u[var[a[k]]], u[var[bb[k]]])
    return b.finish()


def rtype_grid(rtype):
    return rules_grid(6, 7, 8, order="colour_major", seed=3, flags=M.MF_IMPROVEMENT if rtype == M.RTYPE_ADAPTIVE else 0,
                      blocks=3 if rtype in (M.RTYPE_PARTITION, M.RTYPE_OVERLAPPING_PARTITION) else 0)


def directional_grid():
    return band_grid(36, "colour_major", ((-1, 1), (-2, 0), (0, 2)), tails=((2.0, 2.0), (1.5, 3.0), (np.inf, 2.0)), seed=6, shape=(9, 8))


def multipass_grid(order):
    return band_grid(40, order, ((-2, 2), (-1, 0)), seed=31, shape=(14, 10))


def with_bands(m, rng, max_share=1.0):
    """the model with every vector a DIFF factor references overwritten by one with a random band: a random start, a width of up
    to ``max_share`` of the rule's limit (above 1: some fall beyond the rule), tails that may differ"""
    data = m.sh_data.copy()
    for t in sorted({int(t) for t in m.f_table[m.f_kind == M.F_PAIRWISE_DIFF]}):
        n = int(m.sh_dim1[t])
        w = int(rng.integers(0, max(1, int(max_share * n / M.DIFF_BAND_DIV)) + 1))
        lo = int(rng.integers(0, n - min(w, n) + 1))
        D = np.empty(n)
        D[:lo] = rng.choice([0.0, 1.5, 2.0])
        D[lo + w:] = rng.choice([1.5, 2.0, 3.0])
        D[lo:lo + w] = rng.uniform(0.05, 1.0, min(w, n - lo))
        data[int(m.sh_off[t]): int(m.sh_off[t]) + n] = D
    return dataclasses.replace(m, sh_data=data, _keep=[])


def rows_mixed_model():
    return with_bands(T.mixed_graph(np.random.default_rng(41), n=30, max_labels=20, kinds=("diff", "dense")), np.random.default_rng(42))


def mixed_level_grid(order="colour_major"):
    """one truncated and one random vector, alternating over the edges: every level references both"""
    L = 40
    D = np.stack([M.truncated_linear(L, L, 0.2, 0.4), S.u01(2 * L - 1, 77)])
    return S.grid_model(7, 6, L, pairwise="diff", order=order, seed=8, n_tables=2, diff_tables=D)


def mid_grid():
    H, W, L = MID_SIZE
    return band_grid(L, "colour_major", ((-2, 2), (-2, 2)), seed=5, shape=(H, W), n_scales=8)


def fuzz_case(seed):
    """model number ``seed`` of the seeded family: diff_tables_cases.mixed_graph with label counts up to 130 (up to 40 for two in
    three, which keeps the family quick), every DIFF vector with a random band of up to twice the rule's width"""
    rng = np.random.default_rng(57000 + seed)
    scheds = (M.SCHED_LEFT,) if seed % 3 else (M.SCHED_LEFT, M.SCHED_RIGHT, M.SCHED_FULL)
    kinds = ("diff",) if seed % 2 else ("diff", "shared", "dense", "potts")
    big = seed % 3 == 2
    m = T.mixed_graph(rng, scheds=scheds, kinds=kinds, max_labels=130 if big else 40, n=int(rng.integers(6, 16)) if big else None)
    if m.has_diff:
        m = with_bands(m, rng, max_share=float(rng.choice([0.5, 1.0, 2.0])))
    return m, MODES[int(rng.integers(4))], int(rng.integers(2)), rng


def gpu_expansion_cases():
    """(name, model) of EVERY model tests/test_diff_band_gpu.py hands to the oracle as an expansion — the same builders over the
    same parameters.  Left out, with its reason: mid_grid() (compared engine against engine; the oracle never sees it)."""
    for L in GRID_LABELS:
        for order in ORDERS:
            for r in HALF_WIDTHS:
                yield "grid L%d %s r%d" % (L, order, r), label_grid(L, order, r)
    for L in RULE_LABELS:
        for order in ORDERS:
            for extra in (0, 1):
                yield "rule L%d %s +%d" % (L, order, extra), rule_grid(L, order, extra)
    for kind in ASYM_KINDS:
        for L in ASYM_LABELS:
            for order in ORDERS:
                for sc in asym_scale_kinds(kind):
                    yield "asym %s L%d %s %s" % (kind, L, order, sc), asym_grid(kind, L, order, sc)
    for kw in RECT_CHAINS:
        for w in RECT_WIDTHS:
            yield "rect chain %r width %d" % (kw, w), rect_chain(w, **kw)
    for L in TIE_LABELS:
        for order in ORDERS:
            yield "ties L%d %s" % (L, order), ties_grid(L, order)
    for L in PRIMAL_LABELS:
        yield "primal L%d" % L, primal_grid(L, "colour_major")
    for rtype in RTYPES:
        yield "rtype %d" % rtype, rtype_grid(rtype)
    yield "directional", directional_grid()
    for order in ORDERS:
        yield "multipass " + order, multipass_grid(order)
    yield "rows mixed", rows_mixed_model()
    yield "mixed level", mixed_level_grid()
    for s in range(N_FUZZ):
        yield "fuzz %d" % s, fuzz_case(s)[0]


N_GPU_EXPANSIONS = (len(GRID_LABELS) * 2 * len(HALF_WIDTHS) + len(RULE_LABELS) * 4 + sum(len(ASYM_LABELS) * 2 * len(asym_scale_kinds(k)) for k in ASYM_KINDS)
                    + len(RECT_CHAINS) * len(RECT_WIDTHS) + len(TIE_LABELS) * 2 + len(PRIMAL_LABELS) + len(RTYPES) + 1 + 2 + 1 + 1 + N_FUZZ)


@functools.lru_cache(maxsize=None)
def receive_cases():
    """list of (D, d0, d1, scales) of every distinct (vector, dims) a DIFF factor of the GPU models has — mid_grid() included —, with ALL
    the scales its factors carry"""
    seen = {}

    def walk(m):
        if not m.has_diff:
            return
        coff = m.const_offsets()
        for f in np.flatnonzero(m.f_kind == M.F_PAIRWISE_DIFF):
            D = m.shared_table(int(m.f_table[f])).reshape(-1)
            key = (D.tobytes(), int(m.f_dim0[f]), int(m.f_dim1[f]))
            seen.setdefault(key, set()).add(float(m.const_data[coff[f]]))
    for _, m in gpu_expansion_cases():
        walk(m)
    walk(mid_grid())
    return [(np.frombuffer(raw, np.float64), d0, d1, np.array(sorted(sc))) for (raw, d0, d1), sc in seen.items()]
