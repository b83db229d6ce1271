"""Float tables (``table_precision`` f32 / f32_round) in models that also hold SHARED, DIFF and Potts factors: the non-DENSE cells
are gathered into a compact const buffer (host constants) or read from the caller's buffer (``const_dev=``), the SHARED / DIFF cells
{scale offset, table offset} point into whichever it is, and ``upload_costs`` rebuilds all of it.  Models and the yardstick — the
oracle on ``expand(m.with_f32_tables())`` — are in tests/mixed_precision_cases.py; tolerances are those of
tests/test_diff_tables_gpu.py; the re-solve procedure is that of tests/test_recost_gpu.py."""
import dataclasses

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from oracle.binding import Oracle

import mixed_precision_cases as C
import recost_cases as RC

pytestmark = pytest.mark.gpu

LB_RTOL = 1e-5
FLB_ATOL = 1e-12
ANISO, UNIFORM = M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM
MODES = (ANISO, UNIFORM)
ERR_UNSUPPORTED, ERR_STATE = -2, -4
PRECISIONS = ("f32_round", "f32")
STORAGE = ("host", "borrowed")


def _costs(m, prec, seed=None):
    """the model as the cell runs it: arbitrary doubles for f32_round, float-valued costs for the strict mode"""
    if seed is not None:
        return RC.recost(m, seed, float_valued=prec == "f32")
    return C.float_valued(m) if prec == "f32" else m


class Cell:
    """an engine with float tables on ``m`` (host constants or a borrowed device buffer) and the oracle on the yardstick"""

    def __init__(self, m, prec, storage, mode):
        self.m, self.prec, self.storage, self.mode = m, prec, storage, mode
        self.e = E.Engine(0)
        self.const = None
        try:
            self.upload(self.e, m)
        except BaseException:
            self.e.close()
            raise
        self.o = Oracle(C.oracle_model(m)); self.o.set_reparametrization(mode)

    def upload(self, e, m):
        if self.storage == "borrowed":
            import torch
            t = torch.from_numpy(np.ascontiguousarray(m.const_data)).cuda()
            torch.cuda.synchronize()
            e.upload(m, const_dev=t.data_ptr(), keep=(t,), table_precision=self.prec)
            if e is self.e:
                self.const = t
        else:
            e.upload(m, table_precision=self.prec)
        assert e.table_precision() == self.prec
        e.set_reparametrization(self.mode)

    def fresh(self, m):
        f = E.Engine(0)
        try:
            self.upload(f, m)
        except BaseException:
            f.close()
            raise
        return f

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.close()

    def bound(self, what=""):
        lb, lbo = self.e.lower_bound(), self.o.LowerBound()
        assert np.isfinite(lb) and abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (what, lb, lbo)
        return lb

    def duals(self, what=""):
        d, do = self.e.download_duals(), self.o.duals()
        assert not np.any(np.isnan(d)), what
        assert np.array_equal(d, do), (what, float(np.max(np.abs(d - do))))
        return d

    def factor_bounds(self, what=""):
        flb = self.e.factor_lower_bounds()
        ref = np.array([self.o.factor_lower_bound(f) for f in range(self.m.n_factors)])
        assert np.max(np.abs(flb - ref)) <= FLB_ATOL, (what, float(np.max(np.abs(flb - ref))))
        return flb


def _passes_duals_bounds_primal(x, classes=None):
    e, o = x.e, x.o
    if classes is not None:                                        # before anything runs
        for d in (0, 1):
            assert set(e.plan.schedule_classes(d, x.mode)) == classes, e.plan.schedule_classes(d, x.mode)
    x.bound("upload")
    for k in range(3):
        e.compute_pass(1); o.ComputePass(1)
        x.bound(k)
    x.duals()
    x.factor_bounds("tracked")
    e.invalidate_lower_bounds()
    x.factor_bounds("full")
    assert e.lower_bound_recomputed() == x.m.n_factors
    # a rounding pass
    e.compute_pass_and_primal(1); o.ComputePassAndPrimal(1)
    assert np.array_equal(e.download_primal(), o.primal())
    assert e.check_primal_consistency() == o.CheckPrimalConsistency()
    c, co = e.evaluate_primal(), o.EvaluatePrimal()
    assert np.isfinite(co) and abs(c - co) <= 1e-9 * max(1.0, abs(co)), (c, co)
    x.duals("rounding pass")


def _recost_cold_then_warm(x, seed):
    """upload_costs of a recosted B as a cold start (duals given), then of a recosted C as a warm start (constants only); each
    against a fresh engine on the same costs and the oracle, as tests/test_recost_gpu.py _passes / _same do"""
    import torch
    e = x.e
    built, handle = e.schedules_built(), e.plan.h
    assert built > 0
    B = _costs(x.m, x.prec, seed)
    Cm = _costs(x.m, x.prec, seed + 1)
    sf = np.flatnonzero((x.m.f_kind == M.F_PAIRWISE_SHARED) | (x.m.f_kind == M.F_PAIRWISE_DIFF))
    off = x.m.const_offsets()
    assert np.all(B.const_data[off[sf]] != x.m.const_data[off[sf]])          # every scale changes
    for way, new in (("cold", B), ("warm", Cm)):
        if way == "cold":
            if x.storage == "borrowed":                                       # another tensor: copied into the borrowed buffer
                t = torch.from_numpy(np.ascontiguousarray(new.const_data)).cuda(); torch.cuda.synchronize()
                e.upload_costs(const_dev=t.data_ptr(), duals=new.dual_data)
                del t
            else:
                e.upload_costs(const=new.const_data, duals=new.dual_data)
            start = new
        else:
            before = e.download_duals()
            if x.storage == "borrowed":                                       # the same pointer, rewritten in place
                x.const.copy_(torch.from_numpy(np.ascontiguousarray(new.const_data))); torch.cuda.synchronize()
                e.upload_costs(const_dev=x.const.data_ptr())
            else:
                e.upload_costs(const=new.const_data)
            assert np.array_equal(e.download_duals(), before)
            start = dataclasses.replace(new, dual_data=before, _keep=[])
        assert e.plan.h == handle and e.schedules_built() == built
        if x.storage == "borrowed":
            assert np.array_equal(x.const.cpu().numpy(), new.const_data)
        x.m = start
        x.o = Oracle(C.oracle_model(start)); x.o.set_reparametrization(x.mode)
        f = x.fresh(start)
        try:
            for k in range(3):
                e.compute_pass(1); f.compute_pass(1); x.o.ComputePass(1)
                lb = x.bound((way, k))
                assert lb == f.lower_bound(), (way, k)
            d = x.duals(way)
            assert np.array_equal(d, f.download_duals()), way
            flb = x.factor_bounds(way)
            assert np.max(np.abs(flb - f.factor_lower_bounds())) <= FLB_ATOL
        finally:
            f.close()
        assert e.schedules_built() == built


@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_m1_four_kinds_interleaved(prec, storage):
    A = _costs(C.m1(), prec)
    for mode in MODES:
        with Cell(A, prec, storage, mode) as x:
            _passes_duals_bounds_primal(x, C.M1_CLASSES)
            bi = x.e.plan.diff_band_info(0, mode)
            assert 0 < bi["band_launches"] < bi["diff_launches"], bi
            _recost_cold_then_warm(x, 2000 + 10 * mode)


@pytest.mark.parametrize("seed", C.M2_SEEDS)
def test_m2_mixed_neighbourhoods_on_the_generic_class(seed):
    for prec in PRECISIONS:
        for storage in STORAGE:
            A = _costs(C.m2(seed), prec)
            for mode in MODES:
                with Cell(A, prec, storage, mode) as x:
                    assert "generic" in x.e.plan.schedule_classes(0, mode)
                    _passes_duals_bounds_primal(x)
                    _recost_cold_then_warm(x, 3000 + 10 * seed + mode)


@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_stale_bounds_through_the_list_kernel(prec, storage):
    """with eight idle factors per live one, what a pass leaves stale is at most an eighth of all bounds: the list kernel recomputes
    it — float tables, SHARED / DIFF cells and Potts scalars through pw_cost"""
    for base in (C.m1(), C.m2(0)):
        A = _costs(C.with_idle_factors(base), prec)
        with Cell(A, prec, storage, UNIFORM) as x:
            x.bound("upload")
            assert x.e.lower_bound_recomputed() == A.n_factors
            x.e.compute_pass(1); x.o.ComputePass(1)
            x.factor_bounds("list")
            n = x.e.lower_bound_recomputed()
            print("recomputed by the list kernel:", n, "of", A.n_factors)
            assert 0 < n <= A.n_factors // 8
            x.bound("list")
            x.duals()


def test_strict_mode_refuses_then_takes_good_costs():
    """one cell: f32 from host constants.  B with one dense entry that is no float is refused (UNSUPPORTED), everything that would
    read the constants says STATE, then good costs arrive: results equal a fresh engine's, so the scales of the SHARED / DIFF factors
    are B's, not A's"""
    A = _costs(C.m1(), "f32")
    B = _costs(A, "f32", 4001)
    dense = np.flatnonzero(A.f_kind == M.F_PAIRWISE_DENSE)
    k = int(dense[7])
    bad = np.array(B.const_data, copy=True)
    bad[A.const_offsets()[k] + 5] = 0.1                                 # not a float
    with Cell(A, "f32", "host", ANISO) as x:
        e = x.e
        e.compute_pass(2)
        built, handle = e.schedules_built(), e.plan.h
        with pytest.raises(E.EngineError, match=r"factor %d\b" % k) as ei:
            e.upload_costs(const=bad, duals=B.dual_data)
        assert ei.value.code == ERR_UNSUPPORTED
        for call in (lambda: e.compute_pass(1), e.lower_bound, e.factor_lower_bounds):
            with pytest.raises(E.EngineError) as ei:
                call()
            assert ei.value.code == ERR_STATE
        e.upload_costs(const=B.const_data, duals=B.dual_data)
        assert e.plan.h == handle and e.schedules_built() == built
        x.m = B
        x.o = Oracle(C.oracle_model(B)); x.o.set_reparametrization(ANISO)
        f = x.fresh(B)
        try:
            for i in range(3):
                e.compute_pass(1); f.compute_pass(1); x.o.ComputePass(1)
                assert x.bound(i) == f.lower_bound()
            assert np.array_equal(x.duals(), f.download_duals())
            x.factor_bounds()
        finally:
            f.close()
        # A's scales would give other duals: the oracle on A's scales with B's other costs differs
        sf = np.flatnonzero((A.f_kind == M.F_PAIRWISE_SHARED) | (A.f_kind == M.F_PAIRWISE_DIFF))
        mix = np.array(B.const_data, copy=True)
        mix[A.const_offsets()[sf]] = A.const_data[A.const_offsets()[sf]]
        o2 = Oracle(C.oracle_model(dataclasses.replace(B, const_data=mix, _keep=[]))); o2.set_reparametrization(ANISO); o2.ComputePass(3)
        assert not np.array_equal(o2.duals(), x.o.duals())
