"""Models with difference-indexed pairwise factors (F_PAIRWISE_DIFF) used by tests/test_diff_tables_host.py and
tests/test_diff_tables_gpu.py.  The yardstick of every one of them is the CPU oracle on the dense expansion (``expand(m)``: the
oracle is never handed a DIFF or SHARED factor): the host test runs the oracle over every expansion listed here, the GPU test
compares the engine on the DIFF model with it."""
import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

MODES = (M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2, M.REPAM_UNIFORM, M.REPAM_DAMPED_UNIFORM)
ORDERS = ("row_major", "colour_major")
SCALE_KINDS = ("one", "random", "negative", "inf")
# every LDS size class of the kernel (label counts rounded up to 64: 64, 128, ..., 512), with the counts the issue names
GRID_LABELS = (3, 8, 27, 32, 33, 40, 64, 65, 100, 128, 130, 192, 200, 257, 330, 390, 449, 512)
# the label counts whose plans the host test pins
CLASS_LABELS = (3, 8, 27, 32, 33, 40, 64, 100, 130, 512)


def expand(m):
    """the dense model the oracle runs: DIFF factors first, then what SHARED factors a mixed model holds"""
    return m.expand_diff().expand_shared()


def grid_shape(L):
    return (7, 6) if L <= 130 else (4, 3)


def diff_grid(H, W, L, order="row_major", seed=1, n_tables=2, scales="random", compute_primal=False, potential="random"):
    """grid_model(pairwise="diff").  ``scales``: 1.0 everywhere; random in [0.5, 2); one negative; vectors with about 10 % +inf
    entries (the entry of a == b kept finite, so every row and column of the expansion keeps a finite entry), positive scales.
    ``potential``: random vectors (asymmetric), or truncated linear / quadratic ones with a slope and a truncation per vector."""
    E = H * (W - 1) + (H - 1) * W
    kw = dict(pairwise="diff", order=order, seed=seed, n_tables=n_tables, compute_primal=compute_primal)
    if potential == "linear":
        kw["diff_tables"] = np.stack([M.truncated_linear(L, L, 0.1 + 0.05 * t, 0.3 * L * (0.1 + 0.05 * t)) for t in range(n_tables)])
    elif potential == "quadratic":
        kw["diff_tables"] = np.stack([M.truncated_quadratic(L, L, 0.01 + 0.003 * t, 0.7 + 0.1 * t) for t in range(n_tables)])
    elif potential != "random":
        raise ValueError(potential)
    if scales == "random":
        return S.grid_model(H, W, L, **kw)
    if scales == "one":
        return S.grid_model(H, W, L, scales=np.ones(E), **kw)
    if scales == "negative":
        sc = 0.5 + 1.5 * S.u01(E, seed + 77)
        sc[E // 2] = -0.75
        return S.grid_model(H, W, L, scales=sc, **kw)
    if scales == "inf":
        t = S.u01(n_tables * (2 * L - 1), seed + 5).reshape(n_tables, 2 * L - 1)
        hole = S.u01(n_tables * (2 * L - 1), seed + 6).reshape(n_tables, 2 * L - 1) < 0.1
        hole[:, L - 1] = False
        t[hole] = np.inf
        kw["diff_tables"] = t
        return S.grid_model(H, W, L, **kw)
    raise ValueError(scales)


def rect_chain(n=9, seed=3, dims=(5, 9)):
    """chain of variables with label counts da, db, da, ...: rectangular DIFF factors da x db and db x da, a vector each"""
    rng = np.random.default_rng(seed)
    da, db = dims
    # factor types: 0 unary(da), 1 unary(db), 2 pairwise (da, db), 3 pairwise (db, da)
    mt = [M.MsgType(0, 2, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(1, 2, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1),
          M.MsgType(1, 3, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(0, 3, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1)]
    b = M.ModelBuilder(4, mt)
    tab = [b.add_diff_table(rng.uniform(0, 1, da + db - 1)), b.add_diff_table(rng.uniform(0, 1, da + db - 1))]
    u = [int(b.add_vector_factors(i % 2, rng.uniform(0, 1, (1, da if i % 2 == 0 else db)))[0]) for i in range(n)]
    for i in range(n - 1):
        even = i % 2 == 0
        p = int(b.add_diff_pairwise(2 if even else 3, da if even else db, db if even else da, [tab[0 if even else 1]], [rng.uniform(0.5, 2.0)])[0])
        b.add_messages(0 if even else 2, u[i], p)
        b.add_messages(1 if even else 3, u[i + 1], p)
        b.add_relations([u[i], p], [p, u[i + 1]])
    return b.finish()


def rules_grid(H, W, L, order="row_major", seed=1, flags=0, blocks=0, sched=M.SCHED_LEFT, n_tables=2, compute_primal=None):
    """DIFF grid with a message schedule, message-op flags and put_in_same_partition calls of the caller's choice"""
    var = S.grid_variable_order(H, W, order).reshape(-1)
    a, bb = S.grid_edges(H, W)
    i, j = np.minimum(var[a], var[bb]), np.maximum(var[a], var[bb])
    mts = [M.MsgType(0, 1, sched, 0, 1, M.M_UNARY_PAIRWISE, 0, flags), M.MsgType(0, 1, sched, 0, 1, M.M_UNARY_PAIRWISE, 1, flags)]
    b = M.ModelBuilder(2, mts, compute_primal)
    u = b.add_vector_factors(0, S.u01(H * W * L, seed).reshape(-1, L))
    t = [b.add_diff_table(x) for x in S.u01(n_tables * (2 * L - 1), seed + 1).reshape(n_tables, 2 * L - 1)]
    p = b.add_diff_pairwise(1, L, L, np.asarray(t)[np.arange(len(a)) % n_tables], 0.5 + 1.5 * S.u01(len(a), seed + 2))
    b.add_interleaved_messages(np.tile(np.array([0, 1], np.int32), len(a)), np.stack([u[i], u[j]], 1).reshape(-1), np.repeat(p, 2))
    b.add_relations(np.stack([u[i], p], 1).reshape(-1), np.stack([p, u[j]], 1).reshape(-1))
    if blocks:
        band = (np.arange(H * W) % W) * blocks // W
        for k in range(len(a)):
            if band[a[k]] == band[bb[k]]:
                b.put_in_same_partition(u[var[a[k]]], u[var[bb[k]]])
    return b.finish()


def mixed_graph(rng, n=None, max_labels=40, scheds=(M.SCHED_LEFT,), primal=False, kinds=("diff", "shared", "dense", "potts")):
    """random graph, every variable with one of a few label counts, every edge DIFF, SHARED, DENSE or POTTS (Potts between
    variables of equal label counts only), a random subset of the relations u_i -> p -> u_j"""
    n = int(rng.integers(6, 30)) if n is None else n
    counts = sorted({int(x) for x in rng.integers(2, max_labels + 1, size=int(rng.integers(1, 4)))})
    K = len(counts)
    # factor types: k < K unary with counts[k]; K + a * K + b pairwise (counts[a], counts[b])
    mt, mt_of = [], {}
    for a in range(K):
        for c in range(K):
            s0, s1 = int(rng.choice(scheds)), int(rng.choice(scheds))
            mt_of[(a, c)] = len(mt)
            mt.append(M.MsgType(a, K + a * K + c, s0, 0, 1, M.M_UNARY_PAIRWISE, 0))
            mt.append(M.MsgType(c, K + a * K + c, s1, 0, 1, M.M_UNARY_PAIRWISE, 1))
    b = M.ModelBuilder(K + K * K, mt, [1] * K + [0] * (K * K) if primal else None)
    lab = rng.integers(0, K, size=n)
    u = [int(b.add_vector_factors(int(lab[v]), rng.uniform(0, 1, (1, counts[lab[v]])))[0]) for v in range(n)]
    pool, vecs = {}, {}
    rel = []
    for _ in range(int(rng.integers(n, 3 * n))):
        i, j = sorted(int(x) for x in rng.choice(n, 2, replace=False))
        a, c = int(lab[i]), int(lab[j])
        d0, d1 = counts[a], counts[c]
        kind = str(rng.choice(kinds))
        if kind == "potts" and d0 != d1:
            kind = "diff"
        ft = K + a * K + c
        if kind == "diff":
            tabs = vecs.setdefault((d0, d1), [])
            if not tabs or (len(tabs) < 3 and rng.uniform() < 0.3):
                tabs.append(b.add_diff_table(rng.uniform(0, 1, d0 + d1 - 1)))
            p = int(b.add_diff_pairwise(ft, d0, d1, [tabs[int(rng.integers(len(tabs)))]], [rng.uniform(0.5, 2.0)])[0])
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


# pairwise functions 0-1 and 1-2 depend on a - b only (and are bytewise equal); 2-3 (3 x 2) does too; 0-2 does not
UAI_TEXT = """MARKOV
4
3 3 3 2
8
1 0
1 1
1 2
1 3
2 0 1
2 1 2
2 2 3
2 0 2
3 0.1 0.7 0.3
3 0.5 0.2 0.9
3 0.4 0.4 0.1
2 0.6 0.2
9 0.0 1.0 2.0 1.5 0.0 1.0 2.5 1.5 0.0
9 0.0 1.0 2.0 1.5 0.0 1.0 2.5 1.5 0.0
6 0.3 0.9 0.8 0.3 0.5 0.8
9 0.0 1.0 2.0 1.0 0.0 1.0 2.0 1.0 0.25
"""


def fuzz_case(seed):
    """model number ``seed`` of the seeded family: random graphs, label counts <= 130 (<= 40 for three in four, which keeps
    the family quick), a random mix of kinds and schedules"""
    rng = np.random.default_rng(91000 + seed)
    scheds = (M.SCHED_LEFT,) if seed % 3 else (M.SCHED_LEFT, M.SCHED_RIGHT, M.SCHED_FULL)
    kinds = ("diff",) if seed % 4 == 1 else ("diff", "shared", "dense", "potts")
    m = mixed_graph(rng, scheds=scheds, kinds=kinds, max_labels=130 if seed % 4 == 2 else 40, n=int(rng.integers(6, 16)) if seed % 4 == 2 else None)
    return m, MODES[int(rng.integers(4))], int(rng.integers(2)), rng


# ---- the inputs of tests/test_diff_tables_gpu.py, one builder per test and the parameters the test iterates over: the GPU
# tests take their models from here, and gpu_expansion_cases() walks the SAME builders and parameters for the host test -------
RECT_CHAINS = (dict(), dict(n=12, seed=8, dims=(3, 27)), dict(n=7, seed=5, dims=(70, 33)), dict(n=5, seed=6, dims=(40, 200)))
SCALE_SHAPES = ((40, "colour_major"), (13, "row_major"), (100, "colour_major"))
VECTOR_COUNTS = (1, 3, 40)
POTENTIALS = ("linear", "quadratic")
MIXED_SEEDS = tuple(range(6))
UPDATED_SCHEDS = (M.SCHED_RIGHT, M.SCHED_FULL)
UPDATED_LABELS = (3, 8, 20, 40)
RTYPES = (M.RTYPE_SHARED, M.RTYPE_RESIDUAL, M.RTYPE_PARTITION, M.RTYPE_OVERLAPPING_PARTITION, M.RTYPE_ADAPTIVE)
PRIMAL_CASES = ((16, "colour_major"), (40, "row_major"), (130, "colour_major"))
N_FUZZ = 200
MID_SIZE = (256, 256, 64)      # engine against engine on the expansion: no oracle in that test (the expansion is 4 GB of tables)


def label_grid(L, order):
    H, W = grid_shape(L)
    return S.grid_model(H, W, L, pairwise="diff", order=order, seed=L, n_tables=2)


def kernel_name_grid():
    return S.grid_model(7, 6, 40, pairwise="diff", order="colour_major", seed=2)


def asymmetric_grid():
    """D rises on one side of a == b and falls on the other: a transposed read would show"""
    L = 37
    D = np.stack([np.where(np.arange(2 * L - 1) < L - 1, 0.03 * np.arange(2 * L - 1), 2.0 - 0.01 * np.arange(2 * L - 1)),
                  0.002 * np.arange(2 * L - 1, dtype=np.float64) ** 1.5])
    return S.grid_model(6, 5, L, pairwise="diff", order="colour_major", seed=21, diff_tables=D)


def scale_grid(L, order, kind):
    return diff_grid(7, 6, L, order=order, seed=9, scales=kind)


def vectors_grid(n_tables):
    return diff_grid(12, 11, 33, order="colour_major", seed=4, n_tables=n_tables)


def potential_grid(potential):
    return diff_grid(7, 6, 48, order="colour_major", seed=14, potential=potential)


def mixed_case(seed):
    return mixed_graph(np.random.default_rng(300 + seed), n=25)


def updated_pairwise_grid(sched, L):
    return rules_grid(6, 5, L, sched=sched, seed=L)


def directional_grid():
    return S.grid_model(9, 8, 36, pairwise="diff", order="colour_major", seed=6, n_tables=3)


def rtype_grid(rtype):
    return rules_grid(6, 7, 8, order="colour_major", seed=3, flags=M.MF_IMPROVEMENT if rtype == M.RTYPE_ADAPTIVE else 0,
                      blocks=3 if rtype in (M.RTYPE_PARTITION, M.RTYPE_OVERLAPPING_PARTITION) else 0)


def rows_mixed_model():
    return mixed_graph(np.random.default_rng(41), n=30, max_labels=20, kinds=("diff", "dense"))


def rows_plain_grid():
    return S.grid_model(9, 8, 16, pairwise="diff", order="colour_major")


def multipass_grid(order):
    return S.grid_model(14, 10, 40, pairwise="diff", order=order, seed=31)


def speculation_grid():
    return S.grid_model(14, 10, 33, pairwise="diff", order="colour_major", seed=32)


def primal_grid(L, order):
    return diff_grid(6, 5, L, order=order, seed=2, compute_primal=True)


def lower_bound_grid():
    return S.grid_model(9, 8, 70, pairwise="diff", order="colour_major", seed=12)


def stale_bound_models():
    """(name, model, model -> the dense model the oracle gets, table precision): 4 x 4 grids of 5 labels, one per pairwise kind the
    two bound kernels tell apart"""
    kw = dict(order="colour_major", seed=11)
    same = lambda m: m
    return (("dense", S.grid_model(4, 4, 5, **kw), same, None), ("dense_f32", S.grid_model(4, 4, 5, **kw).with_f32_tables(), same, "f32"),
            ("shared", S.grid_model(4, 4, 5, pairwise="shared", n_tables=2, **kw), lambda m: m.expand_shared(), None),
            ("diff", diff_grid(4, 4, 5, order="colour_major", seed=11), expand, None),
            ("potts", S.grid_model(4, 4, 5, pairwise="potts", **kw), same, None))


def uai_model():
    from lp_mp_amd import uai
    return uai.build_lp_from_uai(UAI_TEXT, diff_tables=True).flat_model()


def gpu_expansion_cases():
    """(name, model) of EVERY model tests/test_diff_tables_gpu.py hands to the oracle as an expansion — the same builders over
    the same parameters.  Left out, with its reason: MID_SIZE (compared engine against engine, the oracle never sees it)."""
    for L in GRID_LABELS:
        for order in ORDERS:
            yield "grid L%d %s" % (L, order), label_grid(L, order)
    yield "kernel name grid", kernel_name_grid()
    for kw in RECT_CHAINS:
        yield "rect chain %r" % (kw,), rect_chain(**kw)
    yield "asymmetric", asymmetric_grid()
    for kind in SCALE_KINDS:
        for L, order in SCALE_SHAPES:
            yield "scales %s L%d %s" % (kind, L, order), scale_grid(L, order, kind)
    for nt in VECTOR_COUNTS:
        yield "vectors %d" % nt, vectors_grid(nt)
    for pot in POTENTIALS:
        yield "potential " + pot, potential_grid(pot)
    for seed in MIXED_SEEDS:
        yield "mixed %d" % seed, mixed_case(seed)
    for sched in UPDATED_SCHEDS:
        for L in UPDATED_LABELS:
            yield "schedule %d L%d" % (sched, L), updated_pairwise_grid(sched, L)
    yield "directional", directional_grid()
    for rtype in RTYPES:
        yield "rtype %d" % rtype, rtype_grid(rtype)
    yield "rows mixed", rows_mixed_model()
    yield "rows plain", rows_plain_grid()
    for order in ORDERS:
        yield "multipass " + order, multipass_grid(order)
    yield "speculation", speculation_grid()
    for L, order in PRIMAL_CASES:
        yield "primal L%d %s" % (L, order), primal_grid(L, order)
    yield "lower bounds", lower_bound_grid()
    yield "uai", uai_model()
    for s in range(N_FUZZ):
        yield "fuzz %d" % s, fuzz_case(s)[0]
