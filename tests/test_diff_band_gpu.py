"""The banded form of class ``diff`` on the device (sweep_diff_band_kernel): difference vectors with constant tails.  The yardstick
is the CPU oracle on the dense expansion (``C.expand(m)``) on identical duals, with the tolerances of tests/test_diff_tables_gpu.py:
lower bound within 1e-5 relative after every pass, duals ``np.array_equal`` after the last, per-factor bounds within 1e-12.

Before anything runs every case asserts which kernel its launches are planned on — the banded one for every launch of class diff
where ``C.banded(m)`` (the numpy statement of the rule) says so, none where it does not — and after a timed pass that
``kernel_timing()`` names that kernel."""
import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from oracle.binding import Oracle

import diff_band_cases as C

pytestmark = pytest.mark.gpu

LB_RTOL = 1e-5
FLB_ATOL = 1e-12
MODES = C.MODES
BAND, FULL = "sweep_diff_band_kernel", "sweep_diff_kernel"


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def _planned(eng, mode, banded, only_diff=True):
    """the plan of both sweeps: class diff only, and every one of its launches on the banded kernel — or none"""
    for d in (0, 1):
        if only_diff:
            assert set(eng.plan.schedule_classes(d, mode)) == {"diff"}, eng.plan.schedule_classes(d, mode)
        info = eng.plan.diff_band_info(d, mode)
        assert info["diff_launches"] > 0, info
        assert info["band_launches"] == (info["diff_launches"] if banded else 0), (banded, info)


def _timed(eng, run, banded=True):
    """``run`` under kernel timing: the launches of class diff it issued ran the banded kernel — or none did"""
    eng.enable_kernel_timing(True); eng.reset_kernel_timing()
    run()
    kt = eng.kernel_timing()
    eng.enable_kernel_timing(False)
    assert kt["diff"]["kernel"].startswith(BAND if banded else FULL), kt
    assert kt["diff"]["band_launches"] == (kt["diff"]["launches"] if banded else 0), kt


def _check(eng, m, mode, passes=3, banded=True, only_diff=True, rows_layout=None):
    x = C.expand(m)
    o = Oracle(x)
    o.set_reparametrization(mode)
    eng.upload(m, rows_layout=rows_layout)
    eng.set_reparametrization(mode)
    assert C.banded(m) == banded
    _planned(eng, mode, banded, only_diff)
    lb0, lbo0 = eng.lower_bound(), o.LowerBound()
    assert abs(lb0 - lbo0) <= LB_RTOL * max(1.0, abs(lbo0)), (lb0, lbo0)
    for it in range(passes):
        if it == passes - 1:
            eng.enable_kernel_timing(True); eng.reset_kernel_timing()
        o.ComputePass(1)
        eng.compute_pass(1)
        lb, lbo = eng.lower_bound(), o.LowerBound()
        assert np.isfinite(lb) and abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (lb, lbo)
    kt = eng.kernel_timing()
    eng.enable_kernel_timing(False)
    assert kt["diff"]["kernel"].startswith(BAND if banded else FULL), kt
    assert kt["diff"]["band_launches"] == (kt["diff"]["launches"] if banded else 0), kt
    d, do = eng.download_duals(), o.duals()
    assert not np.any(np.isnan(d))
    assert np.array_equal(d, do), float(np.max(np.abs(d - do)))
    flb = eng.factor_lower_bounds()
    n = min(m.n_factors, 3000)
    oflb = np.array([o.factor_lower_bound(f) for f in range(n)])
    assert np.max(np.abs(flb[:n] - oflb)) <= FLB_ATOL
    return o


# ---- the kernel: every label count, every window ----------------------------------------------------------------------------
@pytest.mark.parametrize("L", C.GRID_LABELS)
@pytest.mark.parametrize("order", C.ORDERS)
def test_grids_every_lds_size_and_lane_layout(eng, L, order):
    for r in C.HALF_WIDTHS:
        m = C.label_grid(L, order, r)
        for mode in MODES:
            _check(eng, m, mode, 3, banded=(2 * r + 1) * M.DIFF_BAND_DIV <= 2 * L - 1)   # (all but 8 labels, half-width 2)


@pytest.mark.parametrize("L", C.RULE_LABELS)
@pytest.mark.parametrize("order", C.ORDERS)
def test_the_widest_admitted_window_and_one_wider(eng, L, order):
    for mode in MODES:
        _check(eng, C.rule_grid(L, order, 0), mode, 3, banded=True)
        _check(eng, C.rule_grid(L, order, 1), mode, 3, banded=False)       # one entry more: the full kernel, the same yardstick


@pytest.mark.parametrize("kind", C.ASYM_KINDS)
@pytest.mark.parametrize("L", C.ASYM_LABELS)
def test_asymmetric_and_clipped_windows(eng, kind, L):
    """a band left of a == b; one that excludes it (windows clipped or empty at both ends, on both sides); unequal finite tails;
    +inf tails (positive scales); a tail on one side only; a constant vector — with scales 1.0, random, one negative, one 0.0"""
    for order in C.ORDERS:
        for sc in C.asym_scale_kinds(kind):
            for mode in MODES:
                _check(eng, C.asym_grid(kind, L, order, sc), mode, 3)


def test_rectangular_chains_both_sides(eng):
    for kw in C.RECT_CHAINS:
        for w in C.RECT_WIDTHS:
            m = C.rect_chain(w, **kw)
            for mode in MODES:
                _check(eng, m, mode, 3)


@pytest.mark.parametrize("L", C.TIE_LABELS)
def test_ties_and_zeros(eng, L):
    for order in C.ORDERS:
        for mode in MODES:
            _check(eng, C.ties_grid(L, order), mode, 3)


# ---- engine features ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", C.PRIMAL_LABELS)
def test_primal_rounding(eng, L):
    m = C.primal_grid(L, "colour_major")
    x = C.expand(m)
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        o = Oracle(x); o.set_reparametrization(mode)
        eng.upload(m); eng.set_reparametrization(mode)
        _planned(eng, mode, True)
        for it in range(3):
            eng.compute_pass_and_primal(it); o.ComputePassAndPrimal(it)
            assert np.array_equal(eng.download_primal(), o.primal()), (mode, it)
            assert np.array_equal(eng.download_duals(), o.duals()), (mode, it)
            assert eng.check_primal_consistency() == o.CheckPrimalConsistency()
            c, co = eng.evaluate_primal(), o.EvaluatePrimal()
            assert (c == co) if np.isinf(co) else abs(c - co) <= 1e-9 * max(1.0, abs(co)), (c, co)
            eng.compute_pass(1); o.ComputePass(1)
        _timed(eng, lambda: eng.compute_pass_and_primal(3)); o.ComputePassAndPrimal(3)     # the primal sweeps too
        assert np.array_equal(eng.download_primal(), o.primal()) and np.array_equal(eng.download_duals(), o.duals()), mode


@pytest.mark.parametrize("rtype", C.RTYPES)
def test_reparametrization_types(rtype):
    m = C.rtype_grid(rtype)
    x = C.expand(m)
    assert C.banded(m)
    e = E.Engine(0)
    try:
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            o = Oracle(x)
            o.set_reparametrization_type(rtype); o.set_reparametrization(mode)
            e.upload(m); e.set_reparametrization_type(rtype); e.set_reparametrization(mode)
            if rtype != M.RTYPE_ADAPTIVE:                 # (the adaptive rule lives in the generic kernels: no launch of class diff)
                _planned(e, mode, True)
            else:
                assert e.plan.diff_band_info(0, mode)["diff_launches"] == 0
            for n in (1, 2):
                o.ComputePass(n)
                if rtype != M.RTYPE_ADAPTIVE:
                    _timed(e, lambda: e.compute_pass(n))
                else:
                    e.compute_pass(n)
                assert np.array_equal(e.download_duals(), o.duals()), (rtype, mode, n)
                lb, lbo = e.lower_bound(), o.LowerBound()
                assert abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo))
    finally:
        e.set_reparametrization_type(0)
        e.close()


def test_directional_and_custom_passes(eng):
    m = C.directional_grid()
    x = C.expand(m)
    mode = M.REPAM_ANISOTROPIC
    o = Oracle(x); o.set_reparametrization(mode)
    eng.upload(m); eng.set_reparametrization(mode)
    _planned(eng, mode, True)
    eng.forward_pass(); o.ComputeForwardPass()
    assert np.array_equal(eng.download_duals(), o.duals())
    eng.backward_pass(); o.ComputeBackwardPass()
    assert np.array_equal(eng.download_duals(), o.duals())
    upd = o.update_order(M.FORWARD)
    sub = np.ascontiguousarray(upd[::2][:40])
    rows = eng.plan.anisotropic_weights(sub)
    eng.compute_pass_custom(sub, *rows); o.compute_pass_custom(sub, *rows)
    assert np.array_equal(eng.download_duals(), o.duals())
    sid = eng.schedule_create(sub, *rows)
    eng.enable_kernel_timing(True); eng.reset_kernel_timing()
    for _ in range(2):
        eng.schedule_run(sid); o.compute_pass_custom(sub, *rows)
    kt = eng.kernel_timing()
    eng.enable_kernel_timing(False)
    eng.schedule_destroy(sid)
    assert kt["diff"]["kernel"].startswith(BAND), kt
    assert np.array_equal(eng.download_duals(), o.duals())
    assert abs(eng.lower_bound() - o.LowerBound()) <= LB_RTOL * max(1.0, abs(o.LowerBound()))


@pytest.mark.parametrize("order", C.ORDERS)
def test_seven_passes_equal_seven_single_passes(order):
    m = C.multipass_grid(order)
    a, b = E.Engine(0), E.Engine(0)
    try:
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            a.upload(m); a.set_reparametrization(mode)
            b.upload(m); b.set_reparametrization(mode)
            _planned(a, mode, True)
            a.compute_pass(7)
            _timed(b, lambda: b.compute_pass(1))
            for _ in range(6):
                b.compute_pass(1)
            assert np.array_equal(a.download_duals(), b.download_duals())
            assert a.lower_bound() == b.lower_bound()
            o = Oracle(C.expand(m)); o.set_reparametrization(mode); o.ComputePass(7)
            assert np.array_equal(a.download_duals(), o.duals())
    finally:
        a.close(); b.close()


def test_rows_layout_with_a_mixed_model(eng):
    m = C.rows_mixed_model()
    assert m.has_diff and np.any(m.f_kind == M.F_PAIRWISE_DENSE)
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        _check(eng, m, mode, 3, only_diff=False, rows_layout=True)
        assert eng.rows_layout
    eng.upload(m, rows_layout=False)


def test_a_level_with_a_banded_and_an_unbanded_vector_runs_the_full_kernel(eng):
    m = C.mixed_level_grid()
    assert M.diff_band_is_banded(m.shared_table(0).reshape(-1)) and not M.diff_band_is_banded(m.shared_table(1).reshape(-1))
    for mode in MODES:
        _check(eng, m, mode, 3, banded=False)


# ---- mid size, engine against engine ----------------------------------------------------------------------------------------
def test_mid_size_against_the_engine_without_the_banded_kernel(eng, monkeypatch):
    m = C.mid_grid()
    H, W, _ = C.MID_SIZE
    mode = M.REPAM_ANISOTROPIC
    monkeypatch.setenv("LPMP_NO_DIFF_BAND", "1")
    ref = E.Engine(0)
    try:
        ref.upload(m); ref.set_reparametrization(mode)          # the switch is read as the model's plan is made
        monkeypatch.delenv("LPMP_NO_DIFF_BAND")
        eng.upload(m); eng.set_reparametrization(mode)
        _planned(eng, mode, True)
        _planned(ref, mode, False)
        assert eng.plan.schedule_classes(0, mode) == {"diff": H * W}
        for e in (eng, ref):
            e.enable_kernel_timing(True); e.reset_kernel_timing()
            e.compute_pass(1)
            kt = e.kernel_timing()
            e.enable_kernel_timing(False)
            assert kt["diff"]["kernel"].startswith(BAND if e is eng else FULL), kt
            e.compute_pass(4)
        assert np.array_equal(eng.download_duals(), ref.download_duals())
        tracked = eng.lower_bound()
        eng.invalidate_lower_bounds()
        full = eng.lower_bound()
        assert abs(tracked - full) <= 1e-9 * max(1.0, abs(full)), (tracked, full)
    finally:
        ref.close()
        eng.upload(C.rtype_grid(M.RTYPE_SHARED))


# ---- a seeded randomised family ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(C.N_FUZZ // 20))
def test_random_models(block):
    """100 models: random graphs, label counts up to 130, a random mix of kinds and schedules, every DIFF vector with a random band
    of random width (some beyond the rule), a random weight mode and send rule each"""
    eng = E.Engine(0)
    n_band = 0
    try:
        for seed in range(20 * block, 20 * block + 20):
            m, mode, rtype, rng = C.fuzz_case(seed)
            x = C.expand(m)
            o = Oracle(x)
            o.set_reparametrization_type(rtype); o.set_reparametrization(mode)
            eng.upload(m)
            eng.set_reparametrization_type(rtype); eng.set_reparametrization(mode)
            info = [eng.plan.diff_band_info(d, mode) for d in (0, 1)]
            n_band += sum(i["band_launches"] for i in info)
            if m.has_diff and C.banded(m):
                assert all(i["band_launches"] == i["diff_launches"] for i in info), (seed, info)
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
        assert n_band > 0
    finally:
        eng.set_reparametrization_type(0)
        eng.close()
