"""Models and numpy statements of the pool-swap / listed-constants tests (tests/test_repool_host.py, tests/test_repool_gpu.py): one
structure, other pairwise parameters.  Models are built once per process and never modified."""
import dataclasses
import functools

import numpy as np

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

import recost_cases as C

# (slope, trunc) of M.truncated_linear(L, L, slope, trunc): the entries below trunc form a window of about 2 * trunc / slope entries
BANDED = (0.05, 0.2)          # a handful of entries
BANDED_2 = (0.1, 0.25)        # another banded width
UNBANDED = (0.01, 0.2)        # about 40 entries: more than a quarter of the 2 L - 1 = 79 at L = 40


def tl(L, slope_trunc):
    return M.truncated_linear(L, L, *slope_trunc)


@functools.lru_cache(maxsize=None)
def diff_grid(L=40, order="colour_major", n_tables=1, H=7, W=6):
    """7 x 6 DIFF grid whose vectors are all the banded truncated-linear one"""
    D = np.stack([tl(L, BANDED)] * n_tables)
    return S.grid_model(H, W, L, pairwise="diff", order=order, seed=5, diff_tables=D)


@functools.lru_cache(maxsize=None)
def shared_grid_small(L, H=7, W=6):
    return S.grid_model(H, W, L, pairwise="shared", order="colour_major", seed=6, n_tables=2)


def pool_of(m, seed, inf_at=None):
    """new values for every entry of m's pool (u01 stream), optionally one +inf entry"""
    sh = 0.125 + S.u01(m.sh_data.shape[0], seed)
    if inf_at is not None:
        sh[inf_at] = np.inf
    return sh


def listed_subset(m, seed, kinds=None, share=3):
    """about a third of the pairwise factors (of the given kinds), in shuffled order"""
    kinds = (M.F_PAIRWISE_DENSE, M.F_PAIRWISE_POTTS, M.F_PAIRWISE_SHARED, M.F_PAIRWISE_DIFF) if kinds is None else kinds
    pw = np.flatnonzero(np.isin(m.f_kind, kinds))
    rng = np.random.default_rng(seed)
    return rng.permutation(pw)[:max(1, len(pw) // share)].astype(np.int32)


def rows_for(m, factors, seed, float_valued=False, stride=None):
    """a [n, stride] source for Engine.set_constants: row i holds const_size(factors[i]) values 0.25 + u, zeros behind them"""
    sizes = m.const_sizes()[factors]
    stride = int(sizes.max()) if stride is None else int(stride)
    rows = np.zeros((len(factors), stride))
    for i, n in enumerate(sizes):
        rows[i, :n] = 0.25 + S.u01(int(n), seed + i)
    if float_valued:
        rows = rows.astype(np.float32).astype(np.float64)
    return rows


SHIFT_KINDS = (M.F_PAIRWISE_DENSE, M.F_PAIRWISE_POTTS, M.F_PAIRWISE_SHARED, M.F_PAIRWISE_DIFF, M.F_PAIRWISE_DIFF_SHIFT)


def listed_subset_shift(m, seed, share=3):
    """``listed_subset`` that lists DIFF_SHIFT factors as well; a model without the kind: ``listed_subset``, to the entry"""
    return listed_subset(m, seed, kinds=SHIFT_KINDS, share=share)


def rows_for_shift(m, factors, seed, float_valued=False, stride=None):
    """``rows_for`` whose row of a DIFF_SHIFT factor is {scale = 0.25 + u, shift = recost_cases.shifts_for}; every other row, and
    every row of a model without the kind, is that of ``rows_for``, to the bit"""
    rows = rows_for(m, factors, seed, float_valued, stride)
    at = np.flatnonzero(m.f_kind[np.asarray(factors, np.int64)] == M.F_PAIRWISE_DIFF_SHIFT)
    if len(at):
        rows[at, 1] = C.shifts_for(m, np.asarray(factors)[at], seed)
    return rows


def with_rows(m, factors, rows):
    """the numpy statement of Engine.set_constants: the model whose packed constants have those rows replaced"""
    off = m.const_offsets()
    const = np.array(m.const_data, np.float64, copy=True)
    for i, f in enumerate(factors):
        assert m.f_kind[f] != M.F_VECTOR
        n = int(off[f + 1] - off[f])
        const[off[f]:off[f + 1]] = rows[i][:n]
    return dataclasses.replace(m, const_data=const, _keep=[])


def with_duals(m, duals):
    return dataclasses.replace(m, dual_data=np.array(duals, np.float64, copy=True), _keep=[])


oracle_model = C.oracle_model
