"""Models of the float-table tests (tests/test_f32_tables_host.py, tests/test_f32_tables_gpu.py): built once per process and
never modified — a test that needs other tables derives a copy."""
import functools

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

MODES = (M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2, M.REPAM_UNIFORM, M.REPAM_DAMPED_UNIFORM)


@functools.lru_cache(maxsize=None)
def grid(H, W, L, order="colour_major", seed=None, compute_primal=False):
    return S.grid_model(H, W, L, order=order, seed=100 + L if seed is None else seed, compute_primal=compute_primal)


@functools.lru_cache(maxsize=None)
def rect_chain(dims=(3, 7, 4, 9, 2)):
    """5 variables with (3, 7, 4, 9, 2) labels: tables 3x7, 7x4, 4x9, 9x2 — odd row lengths, rows that are not 16-byte aligned as floats
    (or a chain of other label counts: (5, 130, 5, 130) is the streaming class with rectangular tables received on both sides)"""
    b = M.ModelBuilder(2, S.mrf_mtypes())
    rng = np.random.default_rng(5)
    u = [b.add_vector_factors(0, rng.uniform(0, 1, (1, d)))[0] for d in dims]
    for i in range(len(dims) - 1):
        p = b.add_dense_pairwise(1, rng.uniform(0, 1, (dims[i], dims[i + 1])))[0]
        b.add_messages(0, u[i], p); b.add_messages(1, u[i + 1], p)
        b.add_relations(u[i], p); b.add_relations(p, u[i + 1])
    return b.finish()


@functools.lru_cache(maxsize=None)
def mixed_graph(n=40, n_edges=90, L=8, seed=7):
    """random graph whose edges are dense and Potts in turn"""
    rng = np.random.default_rng(seed)
    pairs = set()
    while len(pairs) < n_edges:
        a, c = (int(x) for x in rng.integers(0, n, 2))
        if a != c:
            pairs.add((min(a, c), max(a, c)))
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = b.add_vector_factors(0, rng.uniform(0, 1, (n, L)))
    for k, (i, j) in enumerate(sorted(pairs)):
        if k % 2 == 0:
            p = b.add_dense_pairwise(1, rng.uniform(0, 1, (L, L)))[0]
        else:
            p = b.add_potts_pairwise(1, L, [rng.uniform(0, 1)])[0]
        b.add_messages(0, u[i], p); b.add_messages(1, u[j], p)
        b.add_relations(u[i], p); b.add_relations(p, u[j])
    return b.finish()


@functools.lru_cache(maxsize=None)
def scheduled_grid(H, W, L, sched, seed, flags=0, order="colour_major", dims=None, potts=False):
    """grid MRF whose unary-pairwise messages have the given schedule (right / full: the pairwise factors are updated).
    dims: label counts drawn per variable (rectangular tables); potts: Potts factors with couplings of both signs"""
    mt = [M.MsgType(0, 1, sched, 0, 1, M.M_UNARY_PAIRWISE, 0, flags), M.MsgType(0, 1, sched, 0, 1, M.M_UNARY_PAIRWISE, 1, flags)]
    b = M.ModelBuilder(2, mt)
    var = S.grid_variable_order(H, W, order).reshape(-1)
    a, bb = S.grid_edges(H, W)
    i, j = np.minimum(var[a], var[bb]), np.maximum(var[a], var[bb])
    if dims is not None:
        rng = np.random.default_rng(seed)
        d = rng.choice(dims, size=H * W)
        u = np.array([b.add_vector_factors(0, rng.uniform(0, 1, (1, int(x))))[0] for x in d])
        p = np.array([b.add_dense_pairwise(1, rng.uniform(0, 1, (1, int(d[x]), int(d[y]))))[0] for x, y in zip(i, j)])
    else:
        u = b.add_vector_factors(0, S.u01(H * W * L, seed).reshape(-1, L))
        p = (b.add_potts_pairwise(1, L, np.where(S.u01(len(a), seed + 1) < 0.5, -0.5, 0.75)) if potts
             else b.add_dense_pairwise(1, S.u01(len(a) * L * L, seed + 1).reshape(-1, L, L)))
    b.add_interleaved_messages(np.tile(np.array([0, 1], np.int32), len(a)), np.stack([u[i], u[j]], 1).reshape(-1), np.repeat(p, 2))
    b.add_relations(np.stack([u[i], p], 1).reshape(-1), np.stack([p, u[j]], 1).reshape(-1))
    return b.finish()


def with_tables(m, edit):
    """a copy of m whose constants went through edit(const, offsets) in place"""
    import dataclasses
    const = np.array(m.const_data, np.float64, copy=True)
    edit(const, m.const_offsets())
    return dataclasses.replace(m, const_data=const, _keep=[])


def dense_factors(m):
    return np.flatnonzero(m.f_kind == M.F_PAIRWISE_DENSE)
