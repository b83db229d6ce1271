"""``lower_bound()`` at the slice edges of its sum.  The bound is a per-factor kernel, then ``sum_stage_kernel`` over nb <= 1024
contiguous slices, then a host loop over the nb partial sums (engine.cpp, lpmp_lower_bound): one block up to 256 factors, the cap of
1024 slices from 262 144 factors on.  Everywhere else the suite compares the bound at 1e-5 relative, which a dropped or doubled
factor at a slice edge of a large model stays below; here the models are isolated 2-label vector factors whose bound is known
exactly, and the tolerance is the standard error bound of a sum of nf + nb + 1 terms in any order."""
import math

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

pytestmark = pytest.mark.gpu

CONSTANT = 2.5
SIZES = (1, 255, 256, 257, 511, 513, 262143, 262144, 262145, 262144 + 1023, 300001)
U = 2.0 ** -53


def costs(nf, seed):
    """[nf, 2]: ``S.u01`` values mapped to [-1, 1) and moved away from zero by one (1 <= |x| < 2), every 7th factor scaled by a
    power of two.  Why not the plain map with 2^20 everywhere: the test must fail when ONE factor is lost, i.e. every |bound of a
    factor| must exceed the tolerance (nf + 1026) 2^-53 (sum |flb| + 2.5).  Values near zero never do; and with a seventh of the
    factors at 2^20 the sum is about nf / 7 * 2^20 * 1.5, so that the tolerance passes 1 near nf = 250 000 whatever the other
    factors hold.  2^8 above 513 factors keeps it below 1e-3 at 300 001 (test_one_lost_factor_would_show checks every size)."""
    x = 2.0 * S.u01(2 * nf, seed).reshape(nf, 2) - 1.0
    x = x + np.where(x < 0, -1.0, 1.0)
    x[::7] *= 2.0 ** 20 if nf <= 513 else 2.0 ** 8
    return x


def model(nf, seed=None):
    b = M.ModelBuilder(1, [])
    b.add_vector_factors(0, costs(nf, nf if seed is None else seed))
    b.constant = CONSTANT
    return b.finish()


def tolerance(flb):
    """|fl(sum in any order) - sum| <= (n - 1) u sum|x_i| / (1 - (n - 1) u) for n terms (Higham, Accuracy and Stability of Numerical
    Algorithms, 4.2); the terms: nf factor bounds, at most 1024 partial sums re-added, the constant — n <= nf + 1026, and the
    denominator is within 1e-10 of 1 at these sizes, covered by taking n instead of n - 1"""
    return (flb.shape[0] + 1026) * U * (math.fsum(np.abs(flb)) + CONSTANT)


def _check(e, want_flb, recomputed):
    flb = e.factor_lower_bounds()
    assert e.lower_bound_recomputed() == recomputed
    assert np.array_equal(flb, want_flb)
    lb = e.lower_bound()
    exact = math.fsum(flb) + CONSTANT
    tol = tolerance(flb)
    print("nf", flb.shape[0], "lower bound", repr(lb), "exact", repr(exact), "error", abs(lb - exact), "tolerance", tol)
    assert abs(lb - exact) <= tol, (lb, exact, tol)
    return lb


@pytest.mark.parametrize("nf", SIZES)
def test_one_lost_factor_would_show(nf):
    """on the CPU: with these inputs the smallest factor bound is larger than the tolerance, so a sum that drops (or doubles) any one
    factor — a slice edge — cannot pass"""
    flb = costs(nf, nf).min(axis=1)
    assert np.min(np.abs(flb)) > tolerance(flb), (nf, float(np.min(np.abs(flb))), tolerance(flb))
    if nf == 262145:
        x = costs(nf, nf)
        x[_changed(nf)] = costs(len(_changed(nf)), 7)
        flb = x.min(axis=1)
        assert np.min(np.abs(flb)) > tolerance(flb)


@pytest.mark.parametrize("nf", SIZES)
def test_sum_of_the_factor_bounds(nf):
    m = model(nf)
    e = E.Engine(0)
    try:
        e.upload(m)
        _check(e, m.dual_data.reshape(nf, 2).min(axis=1), nf)
    finally:
        e.close()


def _changed(nf):
    """factors on both sides of slice edges (slices of ceil(nf / 1024) factors), the first and the last"""
    per = (nf + 1023) // 1024
    edges = np.arange(per, nf, per)[::37]
    return np.unique(np.concatenate([[0, nf - 1], edges - 1, edges]))


def test_sum_after_set_vectors_through_the_list_kernel():
    nf = 262145
    m = model(nf)
    ch = _changed(nf)
    rows = costs(len(ch), 7)
    e = E.Engine(0)
    try:
        e.upload(m)
        _check(e, m.dual_data.reshape(nf, 2).min(axis=1), nf)
        e.set_vectors(ch, rows)                      # their tracked bounds become NaN: lb_collect_stale_kernel and the list kernel run before the sum
        x = m.dual_data.reshape(nf, 2).copy()
        x[ch] = rows
        assert 0 < len(ch) <= nf // 8
        lb = _check(e, x.min(axis=1), len(ch))
        e.invalidate_lower_bounds()
        assert e.lower_bound() == lb and e.lower_bound_recomputed() == nf
    finally:
        e.close()
