"""Models of the float-table tests beside SHARED, DIFF and Potts factors (tests/test_mixed_precision_host.py,
tests/test_mixed_precision_gpu.py): with ``table_precision`` f32 / f32_round only the DENSE tables become floats; the cells of the
other kinds — Potts scalars, SHARED / DIFF scales — stay doubles, gathered into a compact buffer when the constants come from host
memory, read from the caller's buffer when they are borrowed.

Yardstick: the CPU oracle on ``oracle_model(m)`` = ``expand(m.with_f32_tables())``, in THAT order: with_f32_tables rounds only tables
that are DENSE at that moment, so the expansions of SHARED / DIFF factors stay ``scale * V`` in double, as the device computes them."""
import dataclasses
import functools

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

import diff_tables_cases as DT

H, W = 6, 5
KINDS = ("dense", "shared", "diff", "potts")
LABELS = {"dense": 32, "shared": 32, "diff": 40, "potts": 16}
ORDER = {"dense": "colour_major", "shared": "colour_major", "diff": "row_major", "potts": "colour_major"}
M1_CLASSES = {"dense32", "shared32", "diff", "potts16"}
M2_SEEDS = tuple(range(6))


def oracle_model(m):
    return DT.expand(m.with_f32_tables())


def wrong_order_model(m):
    """rounds the expansions of the SHARED / DIFF factors too: NOT what the device computes"""
    return DT.expand(m).with_f32_tables()


@functools.lru_cache(maxsize=None)
def m1(kinds=KINDS, compute_primal=True):
    """one model of disjoint 6 x 5 grids, one per kind, whose pairwise factors are added interleaved (edge k of every grid, then edge
    k + 1, ...; the Potts factors in pairs): DENSE tables and the other kinds' cells alternate in the packed constants.  Factor types 2 g (unaries of grid g) and
    2 g + 1 (its pairwise factors).  The DIFF grid is in row-major order with the banded vector on the edges that leave an even
    anti-diagonal and the unbanded one on the others: the receives of a level reference one vector only, so that some launches of
    class diff run the banded kernel and some the full one."""
    G = len(kinds)
    mts = []
    for g in range(G):
        mts += [M.MsgType(2 * g, 2 * g + 1, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(2 * g, 2 * g + 1, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1)]
    b = M.ModelBuilder(2 * G, mts, [1, 0] * G if compute_primal else None)
    a, bb = S.grid_edges(H, W)
    E = len(a)
    grids = []
    for g, kind in enumerate(kinds):
        L = LABELS[kind]
        var = S.grid_variable_order(H, W, ORDER[kind]).reshape(-1)
        u = b.add_vector_factors(2 * g, S.u01(H * W * L, 500 + g).reshape(-1, L))
        i, j = np.minimum(var[a], var[bb]), np.maximum(var[a], var[bb])
        tabs = None
        if kind == "shared":
            tabs = [b.add_shared_table(t) for t in S.u01(2 * L * L, 510 + g).reshape(2, L, L)]
        elif kind == "diff":
            banded, full = M.truncated_linear(L, L, 0.05, 0.15), S.u01(2 * L - 1, 520 + g)
            assert M.diff_band_is_banded(banded) and not M.diff_band_is_banded(full)
            tabs = [b.add_diff_table(banded), b.add_diff_table(full)]
        grids.append((kind, L, u, i, j, tabs))
    diag = np.minimum(a // W + a % W, bb // W + bb % W)          # (row-major: rank = position)
    p = np.empty((G, E), np.int32)
    for k in range(E):
        for g, (kind, L, u, i, j, tabs) in enumerate(grids):
            if kind == "dense":
                p[g, k] = b.add_dense_pairwise(2 * g + 1, S.u01(L * L, 530 + g, k * L * L).reshape(1, L, L))[0]
            elif kind == "shared":
                p[g, k] = b.add_shared_pairwise(2 * g + 1, [tabs[k % 2]], [0.5 + 1.5 * S.u01(1, 540 + g, k)[0]])[0]
            elif kind == "diff":
                p[g, k] = b.add_diff_pairwise(2 * g + 1, L, L, [tabs[int(diag[k]) % 2]], [0.5 + 1.5 * S.u01(1, 550 + g, k)[0]])[0]
            elif k % 2 == 0:
                # Potts factors two at a time behind every second edge: an even number of cells between two DENSE tables, which
                # therefore all start 16-byte aligned in the packed constants (the exact dense class needs that, plan.cpp)
                for q in range(k, min(k + 2, E)):
                    p[g, q] = b.add_potts_pairwise(2 * g + 1, L, [S.u01(1, 560 + g, q)[0]])[0]
    for g, (kind, L, u, i, j, tabs) in enumerate(grids):
        b.add_interleaved_messages(np.tile(np.array([2 * g, 2 * g + 1], np.int32), E), np.stack([u[i], u[j]], 1).reshape(-1), np.repeat(p[g], 2))
        b.add_relations(np.stack([u[i], p[g]], 1).reshape(-1), np.stack([p[g], u[j]], 1).reshape(-1))
    return b.finish()


@functools.lru_cache(maxsize=None)
def m2(seed):
    """diff_tables_cases.mixed_graph with all four kinds: mixed neighbourhoods, the generic class"""
    return DT.mixed_graph(np.random.default_rng(300 + seed), n=25, primal=True)


def with_idle_factors(m, n=None):
    """``m`` with n isolated 2-label vector factors of a type of their own behind its factors (default: 8 per factor of m).  They are
    never updated, so that after a pass at most an eighth of all tracked bounds is stale: the engine recomputes them with the LIST
    kernel (engine.cpp, compute_factor_lbs), which a small model alone never reaches."""
    n = 8 * m.n_factors if n is None else int(n)
    t = m.n_ftypes
    cat = lambda a, v: np.ascontiguousarray(np.concatenate([a, np.full(n, v, a.dtype)]))
    return dataclasses.replace(
        m, _keep=[], n_ftypes=t + 1, ftype_computes_primal=np.concatenate([np.asarray(m.ftype_computes_primal, np.uint8), np.zeros(1, np.uint8)]),
        f_type=cat(m.f_type, t), f_kind=cat(m.f_kind, M.F_VECTOR), f_flags=cat(m.f_flags, 0), f_dim0=cat(m.f_dim0, 2), f_dim1=cat(m.f_dim1, 0),
        f_table=None if m.f_table is None else cat(np.asarray(m.f_table, np.int32), -1),
        dual_data=np.concatenate([m.dual_data, S.u01(2 * n, 77)]))


def float_valued(m):
    """``m`` with every constant rounded to a float: what the strict mode accepts"""
    return dataclasses.replace(m, const_data=m.const_data.astype(np.float32).astype(np.float64), _keep=[])


def dense_entries(m):
    """(factors, flat indices into const_data) of the DENSE tables"""
    off = m.const_offsets()
    return np.flatnonzero(m.f_kind == M.F_PAIRWISE_DENSE), np.repeat(m.f_kind == M.F_PAIRWISE_DENSE, np.diff(off))
