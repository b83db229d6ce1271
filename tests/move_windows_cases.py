"""Models, moves and numpy helpers of tests/test_move_windows_host.py and tests/test_move_windows_gpu.py (lpmp_move_windows: label
windows that move, duals and shifts carried along on the device).  The yardstick of a move is ``lp_mp_amd.model.move_windows``, the
numpy statement of the rule in include/lpmp_engine.h; the yardstick of the passes after it is the CPU oracle on ``expand_diff()`` of
the moved model, as for every DIFF_SHIFT test."""
import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

import diff_shift_cases as D

ORDERS = D.ORDERS
expand = D.expand
GRID_LABELS = (2, 5, 33, 64, 65, 130, 300, 512)
RECT_DIMS = ((5, 9), (70, 130))
H, W = 6, 5


def grid(L, order, seed=None):
    """the 6 x 5 DIFF_SHIFT grid of diff_shift_cases.label_grid's make: vectors of the lengths 1, 2, 5, L, 2L - 1, 3L, a random shift
    per edge.  Factors 0 ... 29 are the unaries."""
    return D.shift_grid(H, W, L, order=order, seed=L if seed is None else seed)


def unaries(m):
    return np.flatnonzero(m.f_kind == M.F_VECTOR).astype(np.int32)


def deltas(dims, seed):
    """one delta per listed unary of ``dims[i]`` labels: the named cases 0, +-1, +-63, +-64, +-(d - 1), +-d, +-(d + 7) dealt out in turn,
    random values in [-(d + 7), d + 7] behind them; from 130 labels on both signs of a move with 64 <= |delta| < d are forced (the
    in-place hazard: a lane's load reads what another lane's store of the same vector overwrites)"""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, np.int64)
    out = np.empty(dims.shape[0], np.int64)
    for i, d in enumerate(dims):
        d = int(d)
        named = [0, 1, -1, 63, -63, 64, -64, d - 1, -(d - 1), d, -d, d + 7, -(d + 7)]
        out[i] = named[i] if i < len(named) else int(rng.integers(-(d + 7), d + 8))
    big = [i for i, d in enumerate(dims) if d >= 130]
    if len(big) >= 2:
        out[big[-1]] = int(rng.integers(64, int(dims[big[-1]])))
        out[big[-2]] = -int(rng.integers(64, int(dims[big[-2]])))
    return out


def has_hazard(dims, delta):
    dims, delta = np.asarray(dims), np.asarray(delta)
    mid = (np.abs(delta) >= 64) & (np.abs(delta) < dims)
    return bool(np.any(mid & (delta > 0)) and np.any(mid & (delta < 0)))


def cost_pair(m, factors, delta, seed, stride=None, inf=False):
    """(cost_old, cost_new) [n, stride]: the model's unary costs in the old window, and new ones — labels that stay in the window keep
    their cost bit for bit on every second row (the term is skipped there), everything else is random.  ``inf``: a few +inf entries
    at labels that stay, in both arrays (equal entries: carried), none elsewhere"""
    rng = np.random.default_rng(seed)
    off = m.dual_offsets()
    L = int(max(m.f_dim0[f] for f in factors))
    stride = L if stride is None else stride
    old = np.full((len(factors), stride), -7.0)
    new = np.full((len(factors), stride), -9.0)
    for i, f in enumerate(factors):
        d = int(m.f_dim0[f])
        old[i, :d] = m.dual_data[off[f]:off[f] + d]
        new[i, :d] = rng.uniform(0, 1, d)
        x = np.arange(d)
        stay = (x + delta[i] >= 0) & (x + delta[i] < d)
        if i % 2 == 0:
            new[i, :d][stay] = old[i, :d][x[stay] + delta[i]]
        inner = stay & (x + delta[i] > 0) & (x + delta[i] < d - 1)      # (not the end values: labels that enter the window copy those)
        if inf and inner.any() and i % 3 == 0:
            k = x[inner][:: max(1, int(inner.sum()) // 3)]
            old[i, k + delta[i]] = np.inf
            new[i, k] = np.inf
    return old, new


def energy(x, duals, labels):
    """the reparametrised energy of a labelling on a DENSE model ``x`` (expand_diff()) with packed ``duals``, as the list of its terms
    in factor order: theta_u[x_u] per unary, (T[a][b] + m1[a]) + m2[b] per pairwise factor whose unaries the messages name"""
    doff, coff = x.dual_offsets(), x.const_offsets()
    side = {}
    for k in range(x.n_messages):
        side[(int(x.m_right[k]), x.mtypes[int(x.m_type[k])].param)] = int(x.m_left[k])
    terms = []
    for f in range(x.n_factors):
        if x.f_kind[f] == M.F_VECTOR:
            terms.append(duals[doff[f] + labels[f]])
        else:
            d0, d1 = int(x.f_dim0[f]), int(x.f_dim1[f])
            a, b = labels[side[(f, 0)]], labels[side[(f, 1)]]
            terms.append((x.const_data[coff[f] + a * d1 + b] + duals[doff[f] + a]) + duals[doff[f] + d0 + b])
    return np.asarray(terms)


def common_labelling(m, factors, delta, rng):
    """(old labels, new labels) per factor of a random labelling whose ABSOLUTE labels lie in both windows of every listed unary: new
    label x of a listed unary is old label x + delta; an unlisted unary keeps its label.  None when a listed window left its old
    place altogether"""
    old = np.zeros(m.n_factors, np.int64)
    new = np.zeros(m.n_factors, np.int64)
    row = {int(f): i for i, f in enumerate(factors)}
    for f in np.flatnonzero(m.f_kind == M.F_VECTOR):
        d = int(m.f_dim0[f])
        dl = int(delta[row[int(f)]]) if int(f) in row else 0
        lo, hi = max(0, -dl), min(d, d - dl)          # new labels x with 0 <= x + dl < d
        if lo >= hi:
            return None
        new[f] = int(rng.integers(lo, hi))
        old[f] = new[f] + dl
    return old, new


# ---- models for the refusals ---------------------------------------------------------------------------------------------------
def edge_grid(other=None, L=5, seed=3, other_edge=4, extra=None):
    """3 x 3 row-major grid, DIFF_SHIFT edges except edge ``other_edge``, which is of kind ``other`` ("dense", "potts", "diff"; None:
    DIFF_SHIFT as well).  ``extra``: "duplicate" adds the side-0 message of edge 2 a second time; "two_unaries" adds a side-0 message
    from ANOTHER unary into edge 2.  Returns (model, unaries, pairwise factors, (i, j) of every edge)"""
    a, bb = S.grid_edges(3, 3)
    i, j = np.minimum(a, bb), np.maximum(a, bb)
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = b.add_vector_factors(0, S.u01(9 * L, seed).reshape(-1, L))
    lens = (L, 2 * L - 1, 3)
    t = [b.add_diff_table(S.u01(n, seed + 1 + k)) for k, n in enumerate(lens)]
    rng = np.random.default_rng(seed)
    p = []
    for e in range(len(i)):
        sc = float(rng.uniform(0.5, 2.0))
        if e == other_edge and other == "dense":
            f = b.add_dense_pairwise(1, rng.uniform(0, 1, (1, L, L)))
        elif e == other_edge and other == "potts":
            f = b.add_potts_pairwise(1, L, [sc])
        elif e == other_edge and other == "diff":
            f = b.add_diff_pairwise(1, L, L, [t[1]], [sc])
        else:
            f = b.add_diff_shift_pairwise(1, L, L, [t[e % 3]], [sc], [int(rng.integers(-L, L + 1))])
        f = int(f[0])
        p.append(f)
        b.add_messages(0, u[i[e]], f)
        b.add_messages(1, u[j[e]], f)
        b.add_relations([u[i[e]], f], [f, u[j[e]]])
    if extra == "duplicate":
        b.add_messages(0, u[i[2]], p[2])
    elif extra == "two_unaries":
        third = next(int(v) for v in range(9) if v not in (i[2], j[2]))
        b.add_messages(0, u[third], p[2])
    return b.finish(), u, p, list(zip(i.tolist(), j.tolist()))


def labeling_model():
    """a DIFF_SHIFT chain of three two-label unaries, the middle one also the left factor of a labeling message into a factor of four
    labelings.  Returns (model, unaries)"""
    mt = S.mrf_mtypes() + [M.MsgType(0, 2, M.SCHED_LEFT, 0, 1, M.M_LABELING, 0)]
    b = M.ModelBuilder(3, mt)
    b.add_labeling_table([(0,), (1,)], [(0, 0), (0, 1), (1, 0), (1, 1)], (0,))
    u = b.add_vector_factors(0, S.u01(6, 1).reshape(3, 2))
    t = b.add_diff_table(S.u01(3, 2))
    p = b.add_diff_shift_pairwise(1, 2, 2, [t, t], [1.0, 0.5], [1, 0])
    q = int(b.add_vector_factors(2, S.u01(4, 3).reshape(1, 4))[0])
    for e in range(2):
        b.add_messages(0, u[e], p[e]); b.add_messages(1, u[e + 1], p[e])
        b.add_relations([u[e], p[e]], [p[e], u[e + 1]])
    b.add_messages(2, u[1], q)
    b.add_relations([u[1]], [q])
    return b.finish(), u


def two_component_model(L=7, seed=11):
    """a DIFF_SHIFT 3 x 3 grid (factors first) and, in the same model, a chain of four unaries joined by DENSE factors.  Returns
    (model, unaries of the grid, factors of the dense component)"""
    a, bb = S.grid_edges(3, 3)
    i, j = np.minimum(a, bb), np.maximum(a, bb)
    b = M.ModelBuilder(2, S.mrf_mtypes())
    rng = np.random.default_rng(seed)
    u = b.add_vector_factors(0, rng.uniform(0, 1, (9, L)))
    t = [b.add_diff_table(rng.uniform(0, 1, n)) for n in (L, 2 * L - 1, 3)]
    for e in range(len(i)):
        f = int(b.add_diff_shift_pairwise(1, L, L, [t[e % 3]], [rng.uniform(0.5, 2.0)], [int(rng.integers(-L, L + 1))])[0])
        b.add_messages(0, u[i[e]], f); b.add_messages(1, u[j[e]], f)
        b.add_relations([u[i[e]], f], [f, u[j[e]]])
    v = b.add_vector_factors(0, rng.uniform(0, 1, (4, L)))
    other = [int(x) for x in v]
    for e in range(3):
        f = int(b.add_dense_pairwise(1, rng.uniform(0, 1, (1, L, L)))[0])
        other.append(f)
        b.add_messages(0, v[e], f); b.add_messages(1, v[e + 1], f)
        b.add_relations([v[e], f], [f, v[e + 1]])
    return b.finish(), u, other


def stub_window_lp(L=6, n=4, seed=2):
    """an LP of the Python mirror: a chain of ``n`` unaries of L labels joined by diff_shift_pairwise_factors.  Returns (lp, unary
    handles, pairwise handles)"""
    from lp_mp_amd import lp as LPM
    rng = np.random.default_rng(seed)
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.diff_shift_pairwise_factor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    lp = LPM.LP(LPM.FMC("windows", [U, P], [ML, MR]))
    t = lp.add_diff_table(rng.uniform(0, 1, 5))
    u = [lp.add_factor(U, rng.uniform(0, 1, L)) for _ in range(n)]
    p = [lp.add_factor(P, L, L, t, float(rng.uniform(0.5, 2.0)), int(rng.integers(-3, 4))) for _ in range(n - 1)]
    for e in range(n - 1):
        lp.add_message(ML, u[e], p[e]); lp.add_message(MR, u[e + 1], p[e])
        lp.AddFactorRelation(u[e], p[e]); lp.AddFactorRelation(p[e], u[e + 1])
    return lp, u, p
