"""Models with shifted difference-indexed pairwise factors (F_PAIRWISE_DIFF_SHIFT: cost(a, b) = scale * D[clip(a - b + s, 0, n - 1)])
used by tests/test_diff_shift_host.py and tests/test_diff_shift_gpu.py.  The yardstick of every one of them is the CPU oracle on the
dense expansion (``expand(m)``: the oracle is never handed the kind): the host test runs the oracle over every expansion listed
here (``gpu_expansion_cases``), the GPU test compares the engine on the DIFF_SHIFT model with it."""
import dataclasses

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

import diff_tables_cases as D

MODES = D.MODES
ORDERS = D.ORDERS
expand = D.expand
# the LDS size classes of the kernel (label counts rounded up to 64) and the edge between four and two waves (384 | 385)
GRID_LABELS = (3, 33, 64, 65, 130, 200, 384, 385, 512)
SCALE_KINDS = ("negative", "inf")


def grid_shape(L):
    return (7, 6) if L <= 130 else (4, 3)


def n_edges(H, W):
    return H * (W - 1) + (H - 1) * W


def vector_lengths(L):
    """the lengths the GPU tests use at L labels: shorter than any window of differences, the plain DIFF length, longer"""
    return (1, 2, 5, L, 2 * L - 1, 3 * L)


def random_shifts(lengths, L, seed):
    """one shift per edge, uniform in [-(n + L), n + L] for the edge's vector length n, with the named cases forced on edges 3, 4,
    5 and 8: shift 0; d1 - 1 (the shift of a plain DIFF factor); every index clamped to 0; every index clamped to n - 1"""
    lengths = np.asarray(lengths, np.int64)
    rng = np.random.default_rng(seed)
    s = rng.integers(-(lengths + L), lengths + L + 1)
    for e, v in ((3, 0), (4, L - 1), (5, -(int(lengths[min(5, len(s) - 1)]) + L)), (8, int(lengths[min(8, len(s) - 1)]) + L)):
        if e < len(s):
            s[e] = v
    return s


def shift_grid(H, W, L, order="row_major", seed=1, lengths=None, scales=None, compute_primal=False, vectors=None, shifts=None):
    """grid_model(pairwise="diff_shift"): vectors of the given lengths (random, hence asymmetric, unless ``vectors`` gives them),
    edge e uses vector e mod len(lengths), random_shifts"""
    lengths = vector_lengths(L) if lengths is None else tuple(lengths)
    if vectors is None:
        vectors = [S.u01(n, seed + 100 + k) for k, n in enumerate(lengths)]
    E = n_edges(H, W)
    if shifts is None:
        shifts = random_shifts([len(vectors[e % len(vectors)]) for e in range(E)], L, seed + 7)
    return S.grid_model(H, W, L, pairwise="diff_shift", order=order, seed=seed, diff_tables=list(vectors), shifts=shifts, scales=scales,
                        compute_primal=compute_primal)


def label_grid(L, order):
    H, W = grid_shape(L)
    return shift_grid(H, W, L, order=order, seed=L)


def kernel_name_grid():
    return shift_grid(7, 6, 40, order="colour_major", seed=2)


def banded_grid():
    """every vector is a banded truncated-linear one (the plain DIFF grid of these vectors runs the banded kernel)"""
    L = 40
    V = [M.truncated_linear(L, L, 0.2, 0.6), M.truncated_linear(L, L, 0.3, 0.9)]
    assert all(M.diff_band_is_banded(v) for v in V)
    return shift_grid(7, 6, L, order="colour_major", seed=3, vectors=V)


def asymmetric_grid():
    """the vectors of diff_tables_cases.asymmetric_grid (rising on one side of the centre, falling on the other), random shifts: a
    sign error in the index or a transposed read would show"""
    L = 37
    k = np.arange(2 * L - 1)
    V = [np.where(k < L - 1, 0.03 * k, 2.0 - 0.01 * k), 0.002 * k.astype(np.float64) ** 1.5]
    return shift_grid(6, 5, L, order="colour_major", seed=21, vectors=V)


def degenerate_pair(L=40, order="colour_major"):
    """(plain DIFF grid, the DIFF_SHIFT grid with n = d0 + d1 - 1 and s = d1 - 1 on the same vectors and scales)"""
    a = S.grid_model(7, 6, L, pairwise="diff", order=order, seed=9, n_tables=3)
    b = S.grid_model(7, 6, L, pairwise="diff_shift", order=order, seed=9, n_tables=3)
    return a, b


def rect_chain(n=9, seed=3, dims=(5, 9)):
    """chain of variables with label counts da, db, da, ...: rectangular DIFF_SHIFT factors da x db and db x da, vectors of several
    lengths, a random shift each (the unaries sit on both sides of both shapes)"""
    rng = np.random.default_rng(seed)
    da, db = dims
    mt = [M.MsgType(0, 2, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(1, 2, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1),
          M.MsgType(1, 3, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(0, 3, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1)]
    b = M.ModelBuilder(4, mt)
    lens = (da + db - 1, max(da, db), 4, 2 * (da + db))
    tab = [b.add_diff_table(rng.uniform(0, 1, n_)) for n_ in lens]
    u = [int(b.add_vector_factors(i % 2, rng.uniform(0, 1, (1, da if i % 2 == 0 else db)))[0]) for i in range(n)]
    for i in range(n - 1):
        even = i % 2 == 0
        t = i % len(tab)
        s = int(rng.integers(-(lens[t] + max(da, db)), lens[t] + max(da, db) + 1))
        p = int(b.add_diff_shift_pairwise(2 if even else 3, da if even else db, db if even else da, [tab[t]], [rng.uniform(0.5, 2.0)], [s])[0])
        b.add_messages(0 if even else 2, u[i], p)
        b.add_messages(1 if even else 3, u[i + 1], p)
        b.add_relations([u[i], p], [p, u[i + 1]])
    return b.finish()


def scale_grid(L, order, kind):
    """``negative``: one negative scale among random ones.  ``inf``: about 10 % +inf entries, the centre and the two ends of every
    vector finite, vector lengths <= L: the L consecutive indices of a row or column of a factor then hold the whole vector or,
    clamped, one of its ends, so every row and column of every expansion keeps a finite entry whatever the shift"""
    E = n_edges(7, 6)
    if kind == "negative":
        sc = 0.5 + 1.5 * S.u01(E, 86)
        sc[E // 2] = -0.75
        return shift_grid(7, 6, L, order=order, seed=9, scales=sc)
    if kind == "inf":
        lens = (L, 5, 2, max(3, L // 2))
        V = []
        for k, n in enumerate(lens):
            v = S.u01(n, 50 + k)
            hole = S.u01(n, 60 + k) < 0.1
            hole[[0, n // 2, n - 1]] = False
            v[hole] = np.inf
            V.append(v)
        return shift_grid(7, 6, L, order=order, seed=9, vectors=V)
    raise ValueError(kind)


def vectors_grid(n_tables):
    rng = np.random.default_rng(n_tables)
    return shift_grid(12, 11, 33, order="colour_major", seed=4, lengths=[int(x) for x in rng.integers(1, 100, n_tables)])


def mixed_graph(rng, n=None, max_labels=40, scheds=(M.SCHED_LEFT,), kinds=("diff_shift", "diff", "shared", "dense", "potts")):
    """the random graph of diff_tables_cases.mixed_graph with DIFF_SHIFT edges among the others: vectors of any length, one pool
    entry serving factors of several dims and, at times, DIFF and DIFF_SHIFT factors alike"""
    n = int(rng.integers(6, 30)) if n is None else n
    counts = sorted({int(x) for x in rng.integers(2, max_labels + 1, size=int(rng.integers(1, 4)))})
    K = len(counts)
    mt, mt_of = [], {}
    for a in range(K):
        for c in range(K):
            s0, s1 = int(rng.choice(scheds)), int(rng.choice(scheds))
            mt_of[(a, c)] = len(mt)
            mt.append(M.MsgType(a, K + a * K + c, s0, 0, 1, M.M_UNARY_PAIRWISE, 0))
            mt.append(M.MsgType(c, K + a * K + c, s1, 0, 1, M.M_UNARY_PAIRWISE, 1))
    b = M.ModelBuilder(K + K * K, mt)
    lab = rng.integers(0, K, size=n)
    u = [int(b.add_vector_factors(int(lab[v]), rng.uniform(0, 1, (1, counts[lab[v]])))[0]) for v in range(n)]
    pool, vecs, any_len = {}, {}, []
    rel = []
    for _ in range(int(rng.integers(n, 3 * n))):
        i, j = sorted(int(x) for x in rng.choice(n, 2, replace=False))
        a, c = int(lab[i]), int(lab[j])
        d0, d1 = counts[a], counts[c]
        kind = str(rng.choice(kinds))
        if kind == "potts" and d0 != d1:
            kind = "diff_shift"
        ft = K + a * K + c
        if kind == "diff":
            tabs = vecs.setdefault((d0, d1), [])
            if not tabs or (len(tabs) < 3 and rng.uniform() < 0.3):
                tabs.append(b.add_diff_table(rng.uniform(0, 1, d0 + d1 - 1)))
            p = int(b.add_diff_pairwise(ft, d0, d1, [tabs[int(rng.integers(len(tabs)))]], [rng.uniform(0.5, 2.0)])[0])
        elif kind == "diff_shift":
            # a vector of its own length, or one a plain DIFF factor of these dims uses, whatever is there
            own = [t for ts in vecs.values() for t in ts]
            if own and rng.uniform() < 0.3:
                t = own[int(rng.integers(len(own)))]
            else:
                if not any_len or (len(any_len) < 4 and rng.uniform() < 0.4):
                    any_len.append(b.add_diff_table(rng.uniform(0, 1, int(rng.integers(1, 3 * max_labels)))))
                t = any_len[int(rng.integers(len(any_len)))]
            nt = b._shared[t].shape[1]
            s = int(rng.integers(-(nt + max_labels), nt + max_labels + 1))
            p = int(b.add_diff_shift_pairwise(ft, d0, d1, [t], [rng.uniform(0.5, 2.0)], [s])[0])
        elif kind == "shared":
            tabs = pool.setdefault((d0, d1), [])
            if not tabs or (len(tabs) < 3 and rng.uniform() < 0.3):
                tabs.append(b.add_shared_table(rng.uniform(0, 1, (d0, d1))))
            p = int(b.add_shared_pairwise(ft, [tabs[int(rng.integers(len(tabs)))]], [rng.uniform(0.5, 2.0)])[0])
        elif kind == "dense":
            p = int(b.add_dense_pairwise(ft, rng.uniform(0, 1, (1, d0, d1)))[0])
        else:
            p = int(b.add_potts_pairwise(ft, d0, [rng.uniform(-0.5, 1)])[0])
        b.add_messages(mt_of[(a, c)], u[i], p)
        b.add_messages(mt_of[(a, c)] + 1, u[j], p)
        rel += [(u[i], p), (p, u[j])]
    keep = rng.uniform(size=len(rel)) < rng.choice([1.0, 0.9, 0.5])
    r = np.array([x for x, k in zip(rel, keep) if k], np.int32).reshape(-1, 2)
    if r.shape[0]:
        b.add_relations(r[:, 0], r[:, 1])
    b.constant = float(rng.uniform(-1, 1))
    return b.finish()


N_FUZZ = 100
FUZZ_BLOCK = 20


def fuzz_case(seed):
    """model number ``seed`` of the seeded family: random graphs mixing DIFF_SHIFT with DIFF, SHARED, DENSE and POTTS, labels <= 40
    (<= 130 for one seed in four), `left` schedules or a mix of `left` / `right` / `full`, a weight mode and a send rule"""
    rng = np.random.default_rng(77000 + seed)
    scheds = (M.SCHED_LEFT,) if seed % 3 else (M.SCHED_LEFT, M.SCHED_RIGHT, M.SCHED_FULL)
    kinds = ("diff_shift",) if seed % 4 == 1 else ("diff_shift", "diff_shift", "diff", "shared", "dense", "potts")
    big = seed % 4 == 2
    m = mixed_graph(rng, scheds=scheds, kinds=kinds, max_labels=130 if big else 40, n=int(rng.integers(6, 16)) if big else None)
    return m, MODES[int(rng.integers(4))], int(rng.integers(2))


def rules_grid(H, W, L, order="row_major", seed=1, flags=0, blocks=0, sched=M.SCHED_LEFT):
    """DIFF_SHIFT grid with a message schedule, message-op flags and put_in_same_partition calls of the caller's choice"""
    var = S.grid_variable_order(H, W, order).reshape(-1)
    a, bb = S.grid_edges(H, W)
    i, j = np.minimum(var[a], var[bb]), np.maximum(var[a], var[bb])
    mts = [M.MsgType(0, 1, sched, 0, 1, M.M_UNARY_PAIRWISE, 0, flags), M.MsgType(0, 1, sched, 0, 1, M.M_UNARY_PAIRWISE, 1, flags)]
    b = M.ModelBuilder(2, mts)
    u = b.add_vector_factors(0, S.u01(H * W * L, seed).reshape(-1, L))
    lens = (L, 2 * L - 1, 3)
    t = np.asarray([b.add_diff_table(S.u01(n, seed + 1 + k)) for k, n in enumerate(lens)])
    e = np.arange(len(a))
    sh = random_shifts(np.asarray(lens)[e % 3], L, seed + 3)
    p = b.add_diff_shift_pairwise(1, L, L, t[e % 3], 0.5 + 1.5 * S.u01(len(a), seed + 2), sh)
    b.add_interleaved_messages(np.tile(np.array([0, 1], np.int32), len(a)), np.stack([u[i], u[j]], 1).reshape(-1), np.repeat(p, 2))
    b.add_relations(np.stack([u[i], p], 1).reshape(-1), np.stack([p, u[j]], 1).reshape(-1))
    if blocks:
        band = (np.arange(H * W) % W) * blocks // W
        for k in range(len(a)):
            if band[a[k]] == band[bb[k]]:
                b.put_in_same_partition(u[var[a[k]]], u[var[bb[k]]])
    return b.finish()


RECT_CHAINS = (dict(), dict(n=12, seed=8, dims=(3, 27)), dict(n=7, seed=5, dims=(70, 33)), dict(n=5, seed=6, dims=(40, 200)))
SCALE_SHAPES = ((40, "colour_major"), (13, "row_major"))
VECTOR_COUNTS = (1, 3, 40)
UPDATED_SCHEDS = (M.SCHED_RIGHT, M.SCHED_FULL)
UPDATED_LABELS = (3, 8, 40)
RTYPES = D.RTYPES
PRIMAL_CASES = ((16, "colour_major"), (40, "row_major"), (130, "colour_major"))


def updated_pairwise_grid(sched, L):
    return rules_grid(6, 5, L, sched=sched, seed=L)


def rtype_grid(rtype):
    return rules_grid(6, 7, 8, order="colour_major", seed=3, flags=M.MF_IMPROVEMENT if rtype == M.RTYPE_ADAPTIVE else 0,
                      blocks=3 if rtype in (M.RTYPE_PARTITION, M.RTYPE_OVERLAPPING_PARTITION) else 0)


def directional_grid():
    return shift_grid(9, 8, 36, order="colour_major", seed=6)


def multipass_grid(order):
    return shift_grid(14, 10, 40, order=order, seed=31)


def speculation_grid():
    return shift_grid(14, 10, 33, order="colour_major", seed=32)


def layouts_mixed_model(float_valued=False):
    """DENSE beside DIFF_SHIFT (and a few DIFF) factors: the rows layout and float tables move the dense tables and nothing of the
    kind.  ``float_valued``: the dense tables hold floats exactly (table precision f32 accepts them)"""
    m = mixed_graph(np.random.default_rng(41), n=30, max_labels=20, kinds=("diff_shift", "diff_shift", "diff", "dense"))
    return m.with_f32_tables() if float_valued else m


def lower_bound_grid():
    return shift_grid(9, 8, 70, order="colour_major", seed=12)


def primal_grid(L, order):
    return shift_grid(6, 5, L, order=order, seed=2, compute_primal=True)


def recost_grid():
    return shift_grid(7, 6, 40, order="colour_major", seed=15, lengths=(40, 79, 7))


def shift_rows(m, factors, seed):
    """a [n, 2] source for Engine.set_constants on DIFF_SHIFT factors: a new scale AND a new shift per listed factor"""
    rng = np.random.default_rng(seed)
    n = np.asarray([m.sh_dim1[m.f_table[f]] for f in factors], np.int64)
    L = int(m.f_dim0[factors[0]])
    return np.stack([0.25 + rng.uniform(0, 1, len(factors)), rng.integers(-(n + L), n + L + 1).astype(np.float64)], 1)


def with_rows(m, factors, rows):
    """the numpy statement of Engine.set_constants: the model whose packed constants have those rows replaced"""
    off = m.const_offsets()
    const = np.array(m.const_data, np.float64, copy=True)
    for i, f in enumerate(factors):
        const[off[f]:off[f + 1]] = rows[i][:int(off[f + 1] - off[f])]
    return dataclasses.replace(m, const_data=const, _keep=[])


def with_duals(m, duals):
    return dataclasses.replace(m, dual_data=np.array(duals, np.float64, copy=True), _keep=[])


def window_case(seed=5, n_vars=6, full=24, win=7, quadratic=False):
    """(full-range DIFF chain of ``full`` labels on a truncated potential, the windowed DIFF_SHIFT chain of ``win`` labels around
    random centres on the COMPACT vector, the centres)"""
    rng = np.random.default_rng(seed)
    slope, trunc = (0.05, 0.6) if quadratic else (0.2, 0.7)
    Dfull = (M.truncated_quadratic if quadratic else M.truncated_linear)(full, full, slope, trunc)
    Dc, zero = (M.truncated_quadratic_compact if quadratic else M.truncated_linear_compact)(slope, trunc)
    c = rng.integers(0, full - win + 1, n_vars)
    un = rng.uniform(0, 1, (n_vars, full))
    scales = rng.uniform(0.5, 2.0, n_vars - 1)

    def chain(L, add):
        b = M.ModelBuilder(2, S.mrf_mtypes())
        u = b.add_vector_factors(0, un if L == full else np.stack([un[v, c[v]:c[v] + win] for v in range(n_vars)]))
        p = add(b)
        for e in range(n_vars - 1):
            b.add_messages(0, u[e], p[e]); b.add_messages(1, u[e + 1], p[e])
            b.add_relations([u[e], p[e]], [p[e], u[e + 1]])
        return b.finish()
    a = chain(full, lambda b: b.add_diff_pairwise(1, full, full, [b.add_diff_table(Dfull)] * (n_vars - 1), scales))
    w = chain(win, lambda b: b.add_diff_shift_pairwise(1, win, win, [b.add_diff_table(Dc)] * (n_vars - 1), scales, M.window_shift(c[:-1], c[1:], zero)))
    return a, w, c


def gpu_expansion_cases():
    """(name, model) of EVERY model tests/test_diff_shift_gpu.py hands to the oracle as an expansion — the same builders over the same
    parameters"""
    for L in GRID_LABELS:
        for order in ORDERS:
            yield "grid L%d %s" % (L, order), label_grid(L, order)
    yield "kernel name grid", kernel_name_grid()
    yield "banded vectors", banded_grid()
    yield "asymmetric", asymmetric_grid()
    yield "degenerate", degenerate_pair()[1]
    for kw in RECT_CHAINS:
        yield "rect chain %r" % (kw,), rect_chain(**kw)
    for kind in SCALE_KINDS:
        for L, order in SCALE_SHAPES:
            yield "scales %s L%d %s" % (kind, L, order), scale_grid(L, order, kind)
    for nt in VECTOR_COUNTS:
        yield "vectors %d" % nt, vectors_grid(nt)
    for sched in UPDATED_SCHEDS:
        for L in UPDATED_LABELS:
            yield "schedule %d L%d" % (sched, L), updated_pairwise_grid(sched, L)
    yield "directional", directional_grid()
    for rtype in RTYPES:
        yield "rtype %d" % rtype, rtype_grid(rtype)
    yield "layouts mixed", layouts_mixed_model()
    yield "layouts mixed, float tables", layouts_mixed_model(True)
    for order in ORDERS:
        yield "multipass " + order, multipass_grid(order)
    yield "speculation", speculation_grid()
    for L, order in PRIMAL_CASES:
        yield "primal L%d %s" % (L, order), primal_grid(L, order)
    yield "lower bounds", lower_bound_grid()
    yield "recost", recost_grid()
    for s in range(N_FUZZ):
        yield "fuzz %d" % s, fuzz_case(s)[0]
