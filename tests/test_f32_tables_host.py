"""Float storage of dense pairwise tables (lpmp_set_table_precision), the parts that need no GPU: the yardstick model
``FlatModel.with_f32_tables()``, the planner's byte accounting and class routing under the plan-level flag, and the constants."""
import os
import re

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from oracle.binding import Oracle

import f32_tables_cases as C


def test_with_f32_tables_is_the_numpy_round_trip():
    for m in (C.grid(5, 4, 13, "row_major"), C.rect_chain(), C.mixed_graph()):
        x = m.with_f32_tables()
        off = m.const_offsets()
        for f in range(m.n_factors):
            a, b = m.const_data[off[f]:off[f + 1]], x.const_data[off[f]:off[f + 1]]
            if m.f_kind[f] == M.F_PAIRWISE_DENSE:
                assert np.array_equal(b, a.astype(np.float32).astype(np.float64))
            else:
                assert np.array_equal(b, a)                    # Potts scalars stay doubles
        assert np.array_equal(x.dual_data, m.dual_data) and np.array_equal(x.f_kind, m.f_kind)
        assert not np.array_equal(x.const_data, m.const_data)    # (random doubles are not floats)
        assert np.array_equal(x.with_f32_tables().const_data, x.const_data)   # idempotent
    inf = C.with_tables(C.grid(3, 3, 4), lambda c, off: c.__setitem__(slice(5, 9), np.inf))
    assert np.isinf(inf.with_f32_tables().const_data[5:9]).all()


def _dense_table_reads(m, plan, d, mode):
    """dense tables a sweep reads, counted from the plan's weights alone: one per active receive of a unary (its peers are the
    dense factors) and one per updated dense factor that sends anything"""
    upd = plan.update_order(d)
    om_off, om = plan.omega(d, mode)
    mk_off, mk = plan.mask(d, mode)
    n = 0
    for k, f in enumerate(upd):
        if m.f_kind[f] == M.F_VECTOR:
            n += int(np.count_nonzero(mk[mk_off[k]:mk_off[k + 1]]))
        elif m.f_kind[f] == M.F_PAIRWISE_DENSE:
            n += int(np.any(om[om_off[k]:om_off[k + 1]] != 0.0))
    return n


@pytest.mark.parametrize("L", [4, 13, 40, 130])
def test_byte_accounting_and_classes_of_an_f32_plan(L):
    models = [C.grid(4, 3, L, "colour_major"), C.grid(4, 3, L, "row_major")]
    if L <= 32:
        models += [C.scheduled_grid(4, 3, L, M.SCHED_RIGHT, L), C.scheduled_grid(4, 3, L, M.SCHED_FULL, L)]
    for m in models:
        p64, p32 = E.Plan(m), E.Plan(m, table_precision="f32")
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_DAMPED_UNIFORM):
            for d in (M.FORWARD, M.BACKWARD):
                a, b = p64.schedule_info(d, mode), p32.schedule_info(d, mode)
                reads = _dense_table_reads(m, p64, d, mode)
                assert reads > 0
                assert b["algorithmic_bytes"] == a["algorithmic_bytes"] - 4 * L * L * reads, (L, d, mode, reads)
                assert {k: v for k, v in a.items() if k != "algorithmic_bytes"} == {k: v for k, v in b.items() if k != "algorithmic_bytes"}
                assert p64.schedule_classes(d, mode) == p32.schedule_classes(d, mode)
            assert p64.pass_schedule_info(mode)["algorithmic_bytes"] > p32.pass_schedule_info(mode)["algorithmic_bytes"]
    assert E.Plan(models[0], table_precision="f64").schedule_info(0, 0) == E.Plan(models[0]).schedule_info(0, 0)
    assert E.Plan(models[0], table_precision="f32_round").schedule_info(0, 0) == E.Plan(models[0], table_precision="f32").schedule_info(0, 0)
    with pytest.raises(ValueError):
        E.Plan(models[0], table_precision="f16")


def test_the_mode_is_observable_in_the_oracle():
    """the yardstick differs from the f64 model's result: a device path that ignored the mode would be caught"""
    m = C.grid(7, 6, 8)
    a, b = Oracle(m), Oracle(m.with_f32_tables())
    for o in (a, b):
        o.set_reparametrization(M.REPAM_ANISOTROPIC)
        o.ComputePass(3)
    assert not np.array_equal(a.duals(), b.duals())


def test_header_constants_equal_the_python_ones():
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lpmp_engine.h")).read()
    got = {k: int(v) for k, v in re.findall(r"(LPMP_TABLES_\w+)\s*=\s*(\d+)", h)}
    assert got == {"LPMP_TABLES_F64": E.TABLES_F64, "LPMP_TABLES_F32": E.TABLES_F32, "LPMP_TABLES_F32_ROUND": E.TABLES_F32_ROUND}
    assert E.TABLE_PRECISIONS == {"f64": 0, "f32": 1, "f32_round": 2}
    for fn in ("lpmp_set_table_precision", "lpmp_table_precision", "lpmp_plan_set_table_precision"):
        assert re.search(r"\b%s\(" % fn, h) and fn in E.EXPORTS
