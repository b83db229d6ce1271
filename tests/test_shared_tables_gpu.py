"""Shared pairwise tables (F_PAIRWISE_SHARED) on the device.  The yardstick is always ``Oracle(m.expand_shared())`` on identical
duals (the oracle is never handed a SHARED factor), with the tolerances of tests/test_engine_gpu.py: lower bound within 1e-5
relative after every pass, duals ``np.array_equal`` after the last, per-factor bounds within 1e-12.

The shared classes track lower bounds as the dense packed body does (it IS that body with the table fetch replaced): own
factor, pairwise peer after a receive, omega * min(theta) after a forwarded send — ``lower_bound_recomputed`` is 0 after a
uniform-mode pass (test_lower_bounds)."""
import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import shared_tables_cases as C

pytestmark = pytest.mark.gpu

LB_RTOL = 1e-5
FLB_ATOL = 1e-12
MODES = C.MODES
GENERIC = {"generic", "small"}


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(params=[0, 1], ids=["nt0", "nt1"])
def nt_eng(request, monkeypatch):
    monkeypatch.setenv("LPMP_NT", str(request.param))
    e = E.Engine(0)
    e.want_nt = request.param
    yield e
    e.close()


def _check(eng, m, mode, passes=3, only=None, rows_layout=None):
    """``only``: the set of kernel classes the sweep must consist of — asserted BEFORE anything runs, so that the generic
    fallback cannot stand in for the shared classes"""
    x = m.expand_shared()
    o = Oracle(x)
    o.set_reparametrization(mode)
    eng.upload(m, rows_layout=rows_layout)
    eng.set_reparametrization(mode)
    if only is not None:
        for d in (0, 1):
            assert set(eng.plan.schedule_classes(d, mode)) == set(only), (eng.plan.schedule_classes(d, mode), only)
    lb0, lbo0 = eng.lower_bound(), o.LowerBound()
    assert abs(lb0 - lbo0) <= LB_RTOL * max(1.0, abs(lbo0)), (lb0, lbo0)
    for _ in range(passes):
        o.ComputePass(1)
        eng.compute_pass(1)
        lb, lbo = eng.lower_bound(), o.LowerBound()
        assert np.isfinite(lb) and abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (lb, lbo)
    d, do = eng.download_duals(), o.duals()
    assert not np.any(np.isnan(d))
    assert np.array_equal(d, do), float(np.max(np.abs(d - do)))
    flb = eng.factor_lower_bounds()
    n = min(m.n_factors, 3000)
    oflb = np.array([o.factor_lower_bound(f) for f in range(n)])
    assert np.max(np.abs(flb[:n] - oflb)) <= FLB_ATOL
    return o


# ---- the fast class -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", C.FAST_LABELS)
@pytest.mark.parametrize("order", C.ORDERS)
def test_fast_class_grids_both_access_policies(nt_eng, L, order):
    for n_tables in C.FAST_TABLES:
        m = C.fast_grid(L, order, n_tables)
        for mode in MODES:
            _check(nt_eng, m, mode, 3, only={"shared%d" % C.width_of(L)})
            assert nt_eng.L.lpmp_streaming_access(nt_eng.h) == nt_eng.want_nt


def test_fast_class_kernel_name(eng):
    m = C.kernel_name_grid()
    eng.upload(m); eng.set_reparametrization(M.REPAM_ANISOTROPIC)
    eng.enable_kernel_timing(True); eng.reset_kernel_timing()
    eng.compute_pass(2)
    kt = eng.kernel_timing()
    eng.enable_kernel_timing(False)
    assert set(kt) == {"shared32"} and kt["shared32"]["kernel"].startswith("sweep_shared_pk_kernel<32, "), kt
    assert kt["shared32"]["receives"] > 0 and kt["shared32"]["bytes"] > 0


def test_rectangular_tables(eng):
    for kw, cls in C.RECT_CHAINS:
        m = C.rect_chain(**kw)
        for mode in MODES:
            _check(eng, m, mode, 3, only={cls})


@pytest.mark.parametrize("kind", C.SCALE_KINDS)
@pytest.mark.parametrize("mode", [M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM])
def test_scales_and_hard_constraints(eng, kind, mode):
    """scales 1.0; random in [0.5, 2); one negative; tables with +inf entries (positive scales): the oracle runs these
    expansions with finite, increasing bounds and NaN-free duals (tests/test_shared_tables_host.py), so a NaN here is the device's"""
    for L, order in C.SCALE_SHAPES:
        m = C.scale_grid(L, order, kind)
        _check(eng, m, mode, 3, only={"shared%d" % C.width_of(L)})


def test_more_tables_than_the_lds_budget(eng):
    for g in C.BUDGET_GRIDS:
        m = C.budget_grid(*g)
        assert m.n_shared_tables > 4
        for mode in MODES:
            _check(eng, m, mode, 3)


# ---- fallback paths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", C.MIXED_SEEDS)
def test_mixed_neighbourhoods_on_random_graphs(eng, seed):
    m = C.mixed_case(seed)
    for mode in MODES:
        _check(eng, m, mode, 2)


@pytest.mark.parametrize("L", C.BIG_LABELS)
def test_more_than_32_labels(eng, L):
    m = C.big_label_grid(L)
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_DAMPED_UNIFORM):
        _check(eng, m, mode, 2, only={"generic"})


@pytest.mark.parametrize("sched", C.UPDATED_SCHEDS)
@pytest.mark.parametrize("L", C.UPDATED_LABELS)
def test_updated_shared_pairwise_factors(eng, sched, L):
    m = C.updated_pairwise_grid(sched, L)
    for mode in MODES:
        _check(eng, m, mode, 2)
    assert set(eng.plan.schedule_classes(0, M.REPAM_UNIFORM)) & GENERIC


def test_directional_and_custom_passes(eng):
    m = C.directional_grid()
    x = m.expand_shared()
    mode = M.REPAM_ANISOTROPIC
    o = Oracle(x); o.set_reparametrization(mode)
    eng.upload(m); eng.set_reparametrization(mode)
    eng.forward_pass(); o.ComputeForwardPass()
    assert np.array_equal(eng.download_duals(), o.duals())
    eng.backward_pass(); o.ComputeBackwardPass()
    assert np.array_equal(eng.download_duals(), o.duals())
    # an iterator-range pass over a sub-list, once through compute_pass_custom and replayed as a prepared schedule
    upd = o.update_order(M.FORWARD)
    sub = np.ascontiguousarray(upd[::2][:40])
    rows = eng.plan.anisotropic_weights(sub)
    eng.compute_pass_custom(sub, *rows); o.compute_pass_custom(sub, *rows)
    assert np.array_equal(eng.download_duals(), o.duals())
    sid = eng.schedule_create(sub, *rows)
    for _ in range(2):
        eng.schedule_run(sid); o.compute_pass_custom(sub, *rows)
    eng.schedule_destroy(sid)
    assert np.array_equal(eng.download_duals(), o.duals())
    assert abs(eng.lower_bound() - o.LowerBound()) <= LB_RTOL * max(1.0, abs(o.LowerBound()))


@pytest.mark.parametrize("rtype", C.RTYPES)
def test_reparametrization_types(rtype):
    m = C.rtype_grid(rtype)
    x = m.expand_shared()
    e = E.Engine(0)
    try:
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            o = Oracle(x)
            o.set_reparametrization_type(rtype); o.set_reparametrization(mode)
            e.upload(m); e.set_reparametrization_type(rtype); e.set_reparametrization(mode)
            for n in (1, 2):
                o.ComputePass(n); e.compute_pass(n)
                assert np.array_equal(e.download_duals(), o.duals()), (rtype, mode, n)
                lb, lbo = e.lower_bound(), o.LowerBound()
                assert abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo))
    finally:
        e.set_reparametrization_type(0)
        e.close()


def test_rows_layout_with_a_mixed_model(eng):
    m = C.rows_mixed_model()
    assert m.has_shared and np.any(m.f_kind == M.F_PAIRWISE_DENSE)
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        _check(eng, m, mode, 3, rows_layout=True)
        assert eng.rows_layout
    _check(eng, C.rows_plain_grid(), M.REPAM_ANISOTROPIC, 2, rows_layout=True)   # no dense factor at all
    eng.upload(m, rows_layout=False)


# ---- multi-pass calls, speculation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", C.ORDERS)
def test_seven_passes_equal_seven_single_passes(order):
    m = C.multipass_grid(order)
    a, b = E.Engine(0), E.Engine(0)
    try:
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            a.upload(m); a.set_reparametrization(mode)
            b.upload(m); b.set_reparametrization(mode)
            a.compute_pass(7)
            for _ in range(7):
                b.compute_pass(1)
            assert np.array_equal(a.download_duals(), b.download_duals())
            assert a.lower_bound() == b.lower_bound()
            o = Oracle(m.expand_shared()); o.set_reparametrization(mode); o.ComputePass(7)
            assert np.array_equal(a.download_duals(), o.duals())
    finally:
        a.close(); b.close()


def test_speculation_changes_nothing():
    m = C.speculation_grid()
    a, b = E.Engine(0), E.Engine(0)
    try:
        a.upload(m); a.set_reparametrization(M.REPAM_ANISOTROPIC)
        b.upload(m); b.set_reparametrization(M.REPAM_ANISOTROPIC)
        b.set_speculation(8)
        for _ in range(12):
            a.compute_pass(1); b.compute_pass(1)
            assert a.lower_bound() == b.lower_bound()
        assert np.array_equal(a.download_duals(), b.download_duals())
        o = Oracle(m.expand_shared()); o.set_reparametrization(M.REPAM_ANISOTROPIC); o.ComputePass(12)
        assert np.array_equal(a.download_duals(), o.duals())
    finally:
        a.close(); b.close()


# ---- primal ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,order", C.PRIMAL_CASES)
def test_primal_rounding(eng, L, order):
    m = C.primal_grid(L, order)
    x = m.expand_shared()
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        o = Oracle(x); o.set_reparametrization(mode)
        eng.upload(m); eng.set_reparametrization(mode)
        assert set(eng.plan.schedule_classes(0, mode)) == {"shared%d" % C.width_of(L)}
        for it in range(3):
            eng.compute_pass_and_primal(it); o.ComputePassAndPrimal(it)
            assert np.array_equal(eng.download_primal(), o.primal()), (mode, it)
            assert np.array_equal(eng.download_duals(), o.duals()), (mode, it)
            assert eng.check_primal_consistency() == o.CheckPrimalConsistency()
            c, co = eng.evaluate_primal(), o.EvaluatePrimal()
            assert (c == co) if np.isinf(co) else abs(c - co) <= 1e-9 * max(1.0, abs(co)), (c, co)
            eng.compute_pass(1); o.ComputePass(1)


# ---- lower bounds -----------------------------------------------------------------------------------------------------------
def test_lower_bounds(eng):
    m = C.lower_bound_grid()
    x = m.expand_shared()
    o = Oracle(x); o.set_reparametrization(M.REPAM_UNIFORM)
    eng.upload(m); eng.set_reparametrization(M.REPAM_UNIFORM)

    def same():
        lb, lbo = eng.lower_bound(), o.LowerBound()
        assert abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (lb, lbo)
        flb = eng.factor_lower_bounds()
        assert np.max(np.abs(flb - np.array([o.factor_lower_bound(f) for f in range(m.n_factors)]))) <= FLB_ATOL
    same()                                              # right after the upload
    d = np.random.default_rng(3).uniform(-1, 1, m.dual_data.shape[0])
    eng.upload_duals(d)
    import dataclasses
    o = Oracle(dataclasses.replace(x, dual_data=d.copy(), _keep=[]))
    o.set_reparametrization(M.REPAM_UNIFORM)
    same()                                              # random duals
    eng.invalidate_lower_bounds()
    eng.lower_bound()
    assert eng.lower_bound_recomputed() == m.n_factors
    same()
    # the shared classes track every bound in the weight modes in which every message is received and then sent
    eng.compute_pass(1); o.ComputePass(1)
    eng.lower_bound()
    assert eng.lower_bound_recomputed() == 0
    same()


# ---- mid size, engine against engine ----------------------------------------------------------------------------------------
def test_mid_size_against_the_expansion_on_the_same_engine(eng):
    m = S.grid_model(*C.MID_SIZE, pairwise="shared", order="colour_major")
    out = []
    for model in (m, m.expand_shared()):
        eng.upload(model); eng.set_reparametrization(M.REPAM_ANISOTROPIC)
        if model is m:
            assert eng.plan.schedule_classes(0, M.REPAM_ANISOTROPIC) == {"shared32": C.MID_SIZE[0] * C.MID_SIZE[1]}
        lbs = []
        for _ in range(10):
            eng.compute_pass(1)
            lbs.append(eng.lower_bound())
        out.append((eng.download_duals(), lbs))
    assert np.array_equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        assert abs(a - b) <= LB_RTOL * max(1.0, abs(b))


# ---- the LP mirror and the UAI reader -------------------------------------------------------------------------------------
def test_lp_mirror_quick_start_with_a_shared_table():
    from lp_mp_amd import lp as LPM
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.shared_pairwise_factor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    lp = LPM.LP(LPM.FMC("SRMP", [U, P], [ML, MR]))
    t = lp.add_shared_table([[0.0, 1.0], [1.0, 0.0]])
    u1, u2 = lp.add_factor(U, [0.0, 1.0]), lp.add_factor(U, [1.0, 0.0])
    p = lp.add_factor(P, t, 1.0)
    lp.add_message(ML, u1, p); lp.add_message(MR, u2, p)
    lp.AddFactorRelation(u1, p); lp.AddFactorRelation(p, u2)
    s = LPM.MpRoundingSolver(lp, LPM.StandardVisitor(maxIter=50))
    s.Solve()
    assert s.lower_bound() == 1.0 and s.primal_cost() == 1.0


def test_solve_uai_with_shared_tables():
    from lp_mp_amd import uai
    a = uai.solve_uai(C.UAI_TEXT, maxIter=60)
    b = uai.solve_uai(C.UAI_TEXT, share_tables=True, maxIter=60)
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


# ---- a seeded randomised family ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(C.N_FUZZ // 20))
def test_random_models(block):
    """200 models: random graphs, label counts <= 40, random mix of kinds and schedules, a random weight mode and send rule each"""
    eng = E.Engine(0)
    try:
        for seed in range(20 * block, 20 * block + 20):
            m, mode, rtype, rng = C.fuzz_case(seed)
            x = m.expand_shared()
            o = Oracle(x)
            o.set_reparametrization_type(rtype); o.set_reparametrization(mode)
            eng.upload(m)
            eng.set_reparametrization_type(rtype); eng.set_reparametrization(mode)
            assert abs(eng.lower_bound() - o.LowerBound()) <= 1e-9 * max(1.0, abs(o.LowerBound()))
            eng.compute_pass(2); o.ComputePass(2)
            assert np.array_equal(eng.download_duals(), o.duals()), (seed, "passes")
            eng.forward_pass(); o.ComputeForwardPass()
            eng.compute_pass(1); o.ComputePass(1)
            assert np.array_equal(eng.download_duals(), o.duals()), (seed, "forward + pass")
            lb, lbo = eng.lower_bound(), o.LowerBound()
            assert abs(lb - lbo) <= 1e-9 * max(1.0, abs(lbo)), seed
            flb = eng.factor_lower_bounds()
            ref = np.array([o.factor_lower_bound(f) for f in range(m.n_factors)])
            assert np.max(np.abs(flb - ref)) <= FLB_ATOL, seed
    finally:
        eng.set_reparametrization_type(0)
        eng.close()
