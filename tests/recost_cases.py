"""Models and numpy statements of the re-solve tests (tests/test_recost_host.py, tests/test_recost_gpu.py): one structure, costs from
different seeds.  Models are built once per process and never modified — ``recost`` returns a copy with other cost arrays."""
import dataclasses
import functools

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S


def vector_mask(m):
    """True for the entries of the packed dual array that belong to VECTOR factors"""
    return np.repeat(m.f_kind == M.F_VECTOR, m.dual_sizes())


def recost(m, seed, float_valued=False):
    """the structure of ``m`` with costs of another seed (``S.u01`` streams): every constant 0.25 + u, every vector factor's cost u,
    every message vector +0.0.  The shared pool is structure and stays.  ``float_valued``: constants that are exactly floats."""
    vm = vector_mask(m)
    dual = np.zeros(vm.shape[0], np.float64)
    dual[vm] = S.u01(int(vm.sum()), seed)
    n_const = int(m.const_sizes().sum())
    const = 0.25 + S.u01(n_const, seed + 1)
    if float_valued:
        const = const.astype(np.float32).astype(np.float64)
    return dataclasses.replace(m, const_data=const, dual_data=dual, _keep=[])


def shifts_for(m, factors, seed):
    """one integer shift per listed DIFF_SHIFT factor, uniform in [-(n + L), n + L] (n: length of the factor's vector D, L: its larger
    label count), as doubles; every sixteenth entry — counted from ``seed`` — is a named case: shift 0, every index clamped to 0,
    every index clamped to n - 1"""
    factors = np.asarray(factors, np.int64)
    n = np.asarray(m.sh_dim1, np.int64)[np.asarray(m.f_table)[factors]]
    L = np.maximum(m.f_dim0[factors], m.f_dim1[factors]).astype(np.int64)
    s = np.random.default_rng([int(seed), 6]).integers(-(n + L), n + L + 1)
    k = (int(seed) + np.arange(len(factors))) % 16
    s = np.where(k == 0, 0, np.where(k == 1, -(n + L), np.where(k == 2, n + L, s)))
    return s.astype(np.float64)


def recost_shift(m, seed, float_valued=False):
    """``recost`` for a model that may hold DIFF_SHIFT factors: their rows are {scale = 0.25 + u, shift = shifts_for} (a shift 0.25 + u
    is shift 0 on the device for every factor).  A model without the kind: ``recost``, to the bit."""
    new = recost(m, seed, float_valued)
    fs = np.flatnonzero(m.f_kind == M.F_PAIRWISE_DIFF_SHIFT)
    if len(fs):
        new.const_data[m.const_offsets()[fs] + 1] = shifts_for(m, fs, seed)
    return new


def scatter_rows(m, duals, factors, rows, accumulate=False):
    """the numpy statement of Engine.set_vectors: row i of ``rows`` into (onto) the vector of factors[i] in a copy of the packed duals"""
    off = m.dual_offsets()
    out = np.array(duals, np.float64, copy=True)
    for i, f in enumerate(factors):
        n = int(m.f_dim0[f])
        assert m.f_kind[f] == M.F_VECTOR and off[f + 1] - off[f] == n
        if accumulate:
            out[off[f]:off[f] + n] = out[off[f]:off[f] + n] + rows[i][:n]
        else:
            out[off[f]:off[f] + n] = rows[i][:n]
    return out


def zero_pairwise(m, duals):
    """the numpy statement of Engine.zero_pairwise_duals"""
    out = np.array(duals, np.float64, copy=True)
    out[~vector_mask(m)] = 0.0
    return out


@functools.lru_cache(maxsize=None)
def grid(H, W, L, order="colour_major", pairwise="dense", seed=11, compute_primal=False):
    return S.grid_model(H, W, L, pairwise=pairwise, order=order, seed=seed, compute_primal=compute_primal)


@functools.lru_cache(maxsize=None)
def shared_grid():
    return S.grid_model(13, 11, 32, pairwise="shared", order="colour_major", seed=4, n_tables=2)


@functools.lru_cache(maxsize=None)
def diff_grid(L, banded):
    if banded:
        D = np.stack([M.truncated_linear(L, L, 0.05, 0.2), M.truncated_linear(L, L, 0.02, 0.1)])
        assert all(M.diff_band_is_banded(d) for d in D)
        return S.grid_model(7, 6, L, pairwise="diff", order="colour_major", seed=5, diff_tables=D)
    m = S.grid_model(7, 6, L, pairwise="diff", order="colour_major", seed=5)
    return m


@functools.lru_cache(maxsize=None)
def rows_graph():
    return S.counter_graph_model(300, 1200, 16, 3)


@functools.lru_cache(maxsize=None)
def c5_small():
    return S.c5_model(16, 16, 4, 600, 300, 100, seed=5, window=16, colour_edge_vars=True)


@functools.lru_cache(maxsize=None)
def mailbox_grid():
    return S.grid_model(40, 30, 16, order="row_major", seed=5, compute_primal=True)


@functools.lru_cache(maxsize=None)
def vector_lengths_model():
    """vectors of 1, 3, 63, 64, 65 and 300 labels in a chain: every one has a pairwise neighbour"""
    dims = [1, 3, 63, 64, 65, 300]
    rng = np.random.default_rng(2)
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = [b.add_vector_factors(0, rng.uniform(0, 1, (1, d)))[0] for d in dims]
    for i in range(len(dims) - 1):
        p = b.add_dense_pairwise(1, rng.uniform(0, 1, (dims[i], dims[i + 1])))[0]
        b.add_messages(0, u[i], p); b.add_messages(1, u[i + 1], p)
        b.add_relations(u[i], p); b.add_relations(p, u[i + 1])
    return b.finish()


def oracle_model(m):
    """the model the unchanged CPU oracle runs: SHARED / DIFF factors expanded to private tables"""
    if m.has_shared:
        m = m.expand_shared()
    if m.has_diff:
        m = m.expand_diff()
    return m
