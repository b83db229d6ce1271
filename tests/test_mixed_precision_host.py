"""Float tables beside SHARED, DIFF and Potts factors, on the host: the models of tests/mixed_precision_cases.py plan onto the classes
the GPU test expects, the yardstick's order of operations matters, and a plan made for float tables is the f64 plan with other bytes
for the dense tables only.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mixed_precision_cases as C                # noqa: E402
from lp_mp_amd import engine as E                # noqa: E402
from lp_mp_amd import model as M                 # noqa: E402
from oracle.binding import Oracle                # noqa: E402

MODES = (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM)


def test_m1_interleaves_the_kinds_and_runs_on_the_four_classes():
    m = C.m1()
    pw = m.f_kind[m.f_kind != M.F_VECTOR]
    assert np.array_equal(pw[:9], [M.F_PAIRWISE_DENSE, M.F_PAIRWISE_SHARED, M.F_PAIRWISE_DIFF, M.F_PAIRWISE_POTTS, M.F_PAIRWISE_POTTS,
                                    M.F_PAIRWISE_DENSE, M.F_PAIRWISE_SHARED, M.F_PAIRWISE_DIFF, M.F_PAIRWISE_DENSE])
    assert m.n_shared_tables == 4
    p = E.Plan(m)
    for mode in MODES:
        for d in (0, 1):
            assert set(p.schedule_classes(d, mode)) == C.M1_CLASSES, (mode, d, p.schedule_classes(d, mode))
        bi = p.diff_band_info(0, mode)
        assert 0 < bi["band_launches"] < bi["diff_launches"], bi       # one banded and one unbanded vector on different levels
    x = C.with_idle_factors(m)
    assert x.n_factors == 9 * m.n_factors
    q = E.Plan(x)
    for mode in MODES:
        for d in (0, 1):
            assert q.schedule_classes(d, mode) == p.schedule_classes(d, mode)


@pytest.mark.parametrize("seed", C.M2_SEEDS)
def test_m2_holds_all_four_kinds_and_runs_on_the_generic_class(seed):
    m = C.m2(seed)
    assert {M.F_PAIRWISE_DENSE, M.F_PAIRWISE_POTTS, M.F_PAIRWISE_SHARED, M.F_PAIRWISE_DIFF} <= set(m.f_kind.tolist())
    assert "generic" in E.Plan(m).schedule_classes(0, M.REPAM_ANISOTROPIC)


def test_the_order_of_rounding_and_expanding_matters():
    m = C.m1()
    right, wrong = C.oracle_model(m), C.wrong_order_model(m)
    assert np.array_equal(right.f_kind, wrong.f_kind) and np.all(right.f_kind[right.f_kind != M.F_VECTOR] != M.F_PAIRWISE_SHARED)
    off = right.const_offsets()
    differs = np.array([not np.array_equal(right.const_data[off[f]:off[f + 1]], wrong.const_data[off[f]:off[f + 1]]) for f in range(m.n_factors)])
    was = m.f_kind
    assert not differs[was == M.F_PAIRWISE_DENSE].any() and not differs[was == M.F_PAIRWISE_POTTS].any()
    assert differs[was == M.F_PAIRWISE_SHARED].all() and differs[was == M.F_PAIRWISE_DIFF].all()
    # the expansions of the right order are scale * V in double
    f = int(np.flatnonzero(was == M.F_PAIRWISE_SHARED)[0])
    scale = m.const_data[m.const_offsets()[f]]
    assert np.array_equal(right.const_data[off[f]:off[f + 1]], (np.float64(scale) * m.shared_table(int(m.f_table[f]))).reshape(-1))
    # and the two yardsticks give different duals: the distinction is real
    a, b = Oracle(right), Oracle(wrong)
    for o in (a, b):
        o.set_reparametrization(M.REPAM_ANISOTROPIC); o.ComputePass(2)
    assert not np.array_equal(a.duals(), b.duals())


def test_a_plan_for_float_tables_is_the_f64_plan_with_other_bytes_for_the_dense_tables_only():
    full, dense_only, rest = C.m1(), C.m1(kinds=("dense",)), C.m1(kinds=("shared", "diff", "potts"))
    keys = ("n_levels", "n_launches", "n_receives", "n_sends")

    def bytes_saved(m, mode, d):
        p64, p32 = E.Plan(m), E.Plan(m, table_precision="f32")
        assert p64.schedule_classes(d, mode) == p32.schedule_classes(d, mode)
        a, b = p64.schedule_info(d, mode), p32.schedule_info(d, mode)
        assert [a[k] for k in keys] == [b[k] for k in keys], (a, b)
        assert p64.chain_info(d, mode) == p32.chain_info(d, mode)
        assert p64.diff_band_info(d, mode) == p32.diff_band_info(d, mode)
        pa, pb = p64.pass_schedule_info(mode), p32.pass_schedule_info(mode)
        assert [pa[k] for k in keys] == [pb[k] for k in keys]
        return a["algorithmic_bytes"] - b["algorithmic_bytes"], a["n_receives"]
    for mode in MODES:
        for d in (0, 1):
            saved, _ = bytes_saved(full, mode, d)
            alone, n_recv = bytes_saved(dense_only, mode, d)
            assert bytes_saved(rest, mode, d)[0] == 0                # no dense table: the same bytes
            assert saved == alone == 4 * 32 * 32 * n_recv > 0        # a receive reads its peer's table once: 4 bytes less per entry
