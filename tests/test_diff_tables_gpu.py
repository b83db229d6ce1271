"""Difference-indexed pairwise factors (F_PAIRWISE_DIFF) on the device.  The yardstick is always the CPU oracle on the dense
expansion (``C.expand(m)``: the oracle is never handed a DIFF factor) on identical duals, with the tolerances of
tests/test_engine_gpu.py: lower bound within 1e-5 relative after every pass, duals ``np.array_equal`` after the last,
per-factor bounds within 1e-12.

Class ``diff`` tracks lower bounds as the streaming dense class does (it is that body with the table stream replaced): own
factor, pairwise peer after a receive; a peer that was sent to is recomputed."""
import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import diff_tables_cases as C
import repool_cases as R

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
    fallback cannot stand in for the class"""
    x = C.expand(m)
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


# ---- the class --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", C.GRID_LABELS)
@pytest.mark.parametrize("order", C.ORDERS)
def test_grids_every_lds_size_class_both_access_policies(nt_eng, L, order):
    m = C.label_grid(L, order)
    for mode in MODES:
        _check(nt_eng, m, mode, 3, only={"diff"})
        assert nt_eng.L.lpmp_streaming_access(nt_eng.h) == nt_eng.want_nt


def test_kernel_name(eng):
    m = C.kernel_name_grid()
    eng.upload(m); eng.set_reparametrization(M.REPAM_ANISOTROPIC)
    eng.enable_kernel_timing(True); eng.reset_kernel_timing()
    eng.compute_pass(2)
    kt = eng.kernel_timing()
    eng.enable_kernel_timing(False)
    assert set(kt) == {"diff"} and kt["diff"]["kernel"].startswith("sweep_diff_kernel"), kt
    assert kt["diff"]["receives"] > 0 and kt["diff"]["bytes"] > 0


def test_rectangular_chains_both_sides(eng):
    for kw in C.RECT_CHAINS:
        m = C.rect_chain(**kw)
        for mode in MODES:
            _check(eng, m, mode, 3, only={"diff"})


def test_asymmetric_vectors(eng):
    m = C.asymmetric_grid()
    for mode in MODES:
        _check(eng, m, mode, 3, only={"diff"})


@pytest.mark.parametrize("kind", C.SCALE_KINDS)
@pytest.mark.parametrize("mode", [M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM])
def test_scales_and_hard_constraints(eng, kind, mode):
    """scales 1.0; random in [0.5, 2); one negative; vectors with +inf entries (positive scales): the oracle runs these
    expansions with finite, increasing bounds and NaN-free duals (tests/test_diff_tables_host.py), so a NaN here is the device's"""
    for L, order in C.SCALE_SHAPES:
        _check(eng, C.scale_grid(L, order, kind), mode, 3, only={"diff"})


@pytest.mark.parametrize("n_tables", C.VECTOR_COUNTS)
def test_any_number_of_vectors_in_a_level(eng, n_tables):
    m = C.vectors_grid(n_tables)
    assert m.n_shared_tables == n_tables
    for mode in MODES:
        _check(eng, m, mode, 3, only={"diff"})


@pytest.mark.parametrize("potential", C.POTENTIALS)
def test_truncated_potentials(eng, potential):
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        _check(eng, C.potential_grid(potential), mode, 3, only={"diff"})


# ---- fallback paths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", C.MIXED_SEEDS)
def test_mixed_neighbourhoods_on_random_graphs(eng, seed):
    m = C.mixed_case(seed)
    for mode in MODES:
        _check(eng, m, mode, 2)


@pytest.mark.parametrize("sched", C.UPDATED_SCHEDS)
@pytest.mark.parametrize("L", C.UPDATED_LABELS)
def test_updated_diff_pairwise_factors(eng, sched, L):
    m = C.updated_pairwise_grid(sched, L)
    for mode in MODES:
        _check(eng, m, mode, 2)
    assert set(eng.plan.schedule_classes(0, M.REPAM_UNIFORM)) & GENERIC


def test_directional_and_custom_passes(eng):
    m = C.directional_grid()
    x = C.expand(m)
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
    x = C.expand(m)
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
    assert m.has_diff and np.any(m.f_kind == M.F_PAIRWISE_DENSE)
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
            o = Oracle(C.expand(m)); o.set_reparametrization(mode); o.ComputePass(7)
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
        o = Oracle(C.expand(m)); o.set_reparametrization(M.REPAM_ANISOTROPIC); o.ComputePass(12)
        assert np.array_equal(a.download_duals(), o.duals())
    finally:
        a.close(); b.close()


# ---- primal ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,order", C.PRIMAL_CASES)
def test_primal_rounding(eng, L, order):
    m = C.primal_grid(L, order)
    x = C.expand(m)
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        o = Oracle(x); o.set_reparametrization(mode)
        eng.upload(m); eng.set_reparametrization(mode)
        assert set(eng.plan.schedule_classes(0, mode)) == {"diff"}
        for it in range(3):
            eng.compute_pass_and_primal(it); o.ComputePassAndPrimal(it)
            assert np.array_equal(eng.download_primal(), o.primal()), (mode, it)
            assert np.array_equal(eng.download_duals(), o.duals()), (mode, it)
            assert eng.check_primal_consistency() == o.CheckPrimalConsistency()
            c, co = eng.evaluate_primal(), o.EvaluatePrimal()
            assert (c == co) if np.isinf(co) else abs(c - co) <= 1e-9 * max(1.0, abs(co)), (c, co)
            eng.compute_pass(1); o.ComputePass(1)


# ---- lower bounds -----------------------------------------------------------------------------------------------------------
def test_tracked_lower_bounds_equal_recomputed_ones(eng):
    m = C.lower_bound_grid()
    x = C.expand(m)
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
    # After an anisotropic pass every bound is a tracked one: the backward sweep leaves every pairwise factor with a receive of its
    # earlier unary as the last thing that touched it (bound from that receive's registers), every unary with its own update.
    # The tracked sum against a recomputation of every factor: 1e-9 relative (a receive adds m_s - delta + q in another
    # association than the bound kernel's m_s + q: a few ulp per factor).
    eng.set_reparametrization(M.REPAM_ANISOTROPIC); o.set_reparametrization(M.REPAM_ANISOTROPIC)
    for _ in range(3):
        eng.compute_pass(1); o.ComputePass(1)
        tracked = eng.lower_bound()
        n = eng.lower_bound_recomputed()
        print("factors recomputed after an anisotropic pass:", n)
        assert n == 0
        same()
        eng.invalidate_lower_bounds()
        full = eng.lower_bound()
        assert eng.lower_bound_recomputed() == m.n_factors
        assert abs(tracked - full) <= 1e-9 * max(1.0, abs(full)), (tracked, full)
    # A few stale bounds, every pairwise kind: lower_bound() recomputes just those from the list (factor_lb_list_kernel),
    # factor_lower_bounds() and a bound after invalidate_lower_bounds() recompute every factor (factor_lb_kernel and the packed
    # classes' own).  One device function serves the first two, so the sums are the same double, not merely close.
    for name, model, dense, prec in C.stale_bound_models():
        e = E.Engine(0)
        try:
            e.upload(model, table_precision=prec); e.set_reparametrization(M.REPAM_ANISOTROPIC)
            e.compute_pass(1)
            e.invalidate_lower_bounds(); e.lower_bound()                      # every bound recomputed, none stale
            fs = np.flatnonzero(model.f_kind != M.F_VECTOR)[[1, 7, 18]].astype(np.int32)
            rows = R.rows_for(model, fs, 31, float_valued=prec is not None)
            e.set_constants(fs, rows)                                         # their bounds are stale now
            lb = e.lower_bound()
            k = e.lower_bound_recomputed()
            print(name, "recomputed from the list:", k, "of", model.n_factors)
            assert len(fs) <= k <= model.n_factors // 8, (name, k)          # (more than an eighth stale: everything is recomputed)
            flb = e.factor_lower_bounds()
            e.invalidate_lower_bounds()
            assert lb == e.lower_bound() and e.lower_bound_recomputed() == model.n_factors, name
            o = Oracle(dense(R.with_duals(R.with_rows(model, fs, rows), e.download_duals())))
            assert np.max(np.abs(flb - np.array([o.factor_lower_bound(f) for f in range(model.n_factors)]))) <= FLB_ATOL, name
            assert abs(lb - o.LowerBound()) <= LB_RTOL * max(1.0, abs(o.LowerBound())), name
        finally:
            e.close()


# ---- mid size, engine against engine ----------------------------------------------------------------------------------------
def test_mid_size_against_the_expansion_on_the_same_engine(eng):
    H, W, L = C.MID_SIZE
    m = C.diff_grid(H, W, L, order="colour_major", potential="linear")
    out = []
    for model in (m, m.expand_diff()):
        eng.upload(model); eng.set_reparametrization(M.REPAM_ANISOTROPIC)
        if model is m:
            assert eng.plan.schedule_classes(0, M.REPAM_ANISOTROPIC) == {"diff": H * W}
        lbs = []
        for _ in range(5):
            eng.compute_pass(1)
            lbs.append(eng.lower_bound())
        out.append((eng.download_duals(), lbs))
        eng.upload(C.kernel_name_grid())               # (frees the 4 GB of the expansion)
    assert np.array_equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        assert abs(a - b) <= LB_RTOL * max(1.0, abs(b))


# ---- the LP mirror and the UAI reader -------------------------------------------------------------------------------------
def test_lp_mirror_quick_start_with_a_difference_vector():
    from lp_mp_amd import lp as LPM
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.diff_pairwise_factor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    lp = LPM.LP(LPM.FMC("SRMP", [U, P], [ML, MR]))
    t = lp.add_diff_table(M.truncated_linear(2, 2, 1.0, 5.0))      # the Potts table [[0, 1], [1, 0]]
    u1, u2 = lp.add_factor(U, [0.0, 1.0]), lp.add_factor(U, [1.0, 0.0])
    p = lp.add_factor(P, t, 2, 2, 1.0)
    lp.add_message(ML, u1, p); lp.add_message(MR, u2, p)
    lp.AddFactorRelation(u1, p); lp.AddFactorRelation(p, u2)
    s = LPM.MpRoundingSolver(lp, LPM.StandardVisitor(maxIter=50))
    s.Solve()
    assert s.lower_bound() == 1.0 and s.primal_cost() == 1.0


def test_solve_uai_with_diff_tables():
    from lp_mp_amd import uai
    a = uai.solve_uai(C.UAI_TEXT, maxIter=60)
    b = uai.solve_uai(C.UAI_TEXT, diff_tables=True, maxIter=60)
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


# ---- a seeded randomised family ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(C.N_FUZZ // 20))
def test_random_models(block):
    """200 models: random graphs, label counts up to 130, random mix of kinds and schedules, a random weight mode and send rule each"""
    eng = E.Engine(0)
    try:
        for seed in range(20 * block, 20 * block + 20):
            m, mode, rtype, rng = C.fuzz_case(seed)
            x = C.expand(m)
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
