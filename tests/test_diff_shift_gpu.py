"""Shifted difference-indexed pairwise factors (F_PAIRWISE_DIFF_SHIFT) on the device.  The yardstick is that of
tests/test_diff_tables_gpu.py: the CPU oracle on the dense expansion (``C.expand(m)``: the oracle is never handed the kind) on
identical duals — lower bound within 1e-5 relative after every pass, duals ``np.array_equal`` after the last, per-factor bounds
within 1e-12, kernel classes asserted before anything runs.  The primal paths and the re-cost calls are compared engine against
engine (the expansion, a fresh upload), bit for bit."""
import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from oracle.binding import Oracle

import diff_shift_cases as C

pytestmark = pytest.mark.gpu

LB_RTOL = 1e-5
FLB_ATOL = 1e-12
MODES = C.MODES
GENERIC = {"generic", "small"}
SHIFT = M.F_PAIRWISE_DIFF_SHIFT


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


def _check(eng, m, mode, passes=3, only=None, rows_layout=None, table_precision=None):
    """``only``: the set of kernel classes the sweep must consist of — asserted BEFORE anything runs, so that the generic
    fallback cannot stand in for the class"""
    x = C.expand(m)
    o = Oracle(x)
    o.set_reparametrization(mode)
    eng.upload(m, rows_layout=rows_layout, table_precision=table_precision)
    eng.set_reparametrization(mode)
    if only is not None:
        for d in (0, 1):
            assert set(eng.plan.schedule_classes(d, mode)) == set(only), (eng.plan.schedule_classes(d, mode), only)
            assert eng.plan.diff_band_info(d, mode)["band_launches"] == 0
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
    """vector lengths 1, 2, 5, L, 2L - 1, 3L in one grid; a shift per edge from [-(n + L), n + L] with 0, d1 - 1, all-clamped-low
    and all-clamped-high among them"""
    m = C.label_grid(L, order)
    assert sorted(set(m.sh_dim1)) == sorted(set(C.vector_lengths(L)))
    for mode in MODES:
        _check(nt_eng, m, mode, 3, only={"diff"})
        assert nt_eng.L.lpmp_streaming_access(nt_eng.h) == nt_eng.want_nt


def test_kernel_name(eng):
    for m in (C.kernel_name_grid(), C.banded_grid()):
        eng.upload(m); eng.set_reparametrization(M.REPAM_ANISOTROPIC)
        assert set(eng.plan.schedule_classes(0, M.REPAM_ANISOTROPIC)) == {"diff"}
        eng.enable_kernel_timing(True); eng.reset_kernel_timing()
        eng.compute_pass(2)
        kt = eng.kernel_timing()
        eng.enable_kernel_timing(False)
        assert set(kt) == {"diff"} and kt["diff"]["kernel"] == "sweep_diff_shift_kernel", kt
        assert kt["diff"]["band_launches"] == 0 and kt["diff"]["shift_launches"] == kt["diff"]["launches"] > 0
        assert kt["diff"]["receives"] > 0 and kt["diff"]["bytes"] > 0
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        _check(eng, C.banded_grid(), mode, 3, only={"diff"})


def test_degenerate_model_equals_the_plain_diff_model_bit_for_bit(eng):
    a, b = C.degenerate_pair()
    for mode in MODES:
        out = []
        for m in (a, b):
            eng.upload(m); eng.set_reparametrization(mode)
            assert set(eng.plan.schedule_classes(0, mode)) == {"diff"}
            eng.compute_pass(3)
            out.append((eng.download_duals(), eng.lower_bound(), eng.factor_lower_bounds()))
        assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and np.array_equal(out[0][2], out[1][2])
    _check(eng, b, M.REPAM_ANISOTROPIC, 2, only={"diff"})


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
    for L, order in C.SCALE_SHAPES:
        _check(eng, C.scale_grid(L, order, kind), mode, 3, only={"diff"})


@pytest.mark.parametrize("n_tables", C.VECTOR_COUNTS)
def test_any_number_of_vectors_in_a_level(eng, n_tables):
    m = C.vectors_grid(n_tables)
    assert m.n_shared_tables == n_tables
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        _check(eng, m, mode, 3, only={"diff"})


# ---- fallback paths, send rules, other passes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", C.UPDATED_SCHEDS)
@pytest.mark.parametrize("L", C.UPDATED_LABELS)
def test_updated_pairwise_factors(eng, sched, L):
    m = C.updated_pairwise_grid(sched, L)
    for mode in MODES:
        _check(eng, m, mode, 2)
    assert set(eng.plan.schedule_classes(0, M.REPAM_UNIFORM)) & GENERIC


@pytest.mark.parametrize("rtype", C.RTYPES)
def test_send_rules(rtype):
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


def test_rows_layout_and_float_tables_with_a_mixed_model(eng):
    m = C.layouts_mixed_model()
    assert np.any(m.f_kind == SHIFT) and np.any(m.f_kind == M.F_PAIRWISE_DENSE)
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        _check(eng, m, mode, 3, rows_layout=True)
        assert eng.rows_layout
    eng.upload(m, rows_layout=False)
    mf = C.layouts_mixed_model(float_valued=True)
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        _check(eng, mf, mode, 3, table_precision="f32")
        assert eng.table_precision() == "f32"
    eng.upload(m, table_precision="f64")


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


# ---- lower bounds -------------------------------------------------------------------------------------------------------------
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
    same()
    d = np.random.default_rng(3).uniform(-1, 1, m.dual_data.shape[0])
    eng.upload_duals(d)
    o = Oracle(C.with_duals(x, d)); o.set_reparametrization(M.REPAM_UNIFORM)
    same()
    eng.invalidate_lower_bounds()
    eng.lower_bound()
    assert eng.lower_bound_recomputed() == m.n_factors
    same()
    eng.set_reparametrization(M.REPAM_ANISOTROPIC); o.set_reparametrization(M.REPAM_ANISOTROPIC)
    for _ in range(3):
        eng.compute_pass(1); o.ComputePass(1)
        tracked = eng.lower_bound()
        assert eng.lower_bound_recomputed() == 0           # every bound is a tracked one after an anisotropic pass
        same()
        eng.invalidate_lower_bounds()
        full = eng.lower_bound()
        assert eng.lower_bound_recomputed() == m.n_factors
        # (a receive adds m_s - delta + q in another association than the bound kernel's m_s + q: a few ulp per factor)
        assert abs(tracked - full) <= 1e-9 * max(1.0, abs(full)), (tracked, full)
    # a few stale bounds: lower_bound() recomputes just those from the list (factor_lb_list_kernel); one device function serves
    # both bound kernels, so the sums are the same double
    fs = np.flatnonzero(m.f_kind == SHIFT)[[1, 7, 18]].astype(np.int32)
    rows = C.shift_rows(m, fs, 31)
    eng.invalidate_lower_bounds(); eng.lower_bound()
    eng.set_constants(fs, rows)
    lb = eng.lower_bound()
    k = eng.lower_bound_recomputed()
    assert len(fs) <= k <= m.n_factors // 8, k
    flb = eng.factor_lower_bounds()
    eng.invalidate_lower_bounds()
    assert lb == eng.lower_bound() and eng.lower_bound_recomputed() == m.n_factors
    o = Oracle(C.expand(C.with_duals(C.with_rows(m, fs, rows), eng.download_duals())))
    assert np.max(np.abs(flb - np.array([o.factor_lower_bound(f) for f in range(m.n_factors)]))) <= FLB_ATOL
    assert abs(lb - o.LowerBound()) <= LB_RTOL * max(1.0, abs(o.LowerBound()))


# ---- primal paths: the engine on the model against the same engine on its dense expansion, bit for bit ----------------------------
@pytest.mark.parametrize("L,order", C.PRIMAL_CASES)
def test_primal_paths_equal_the_expansions(L, order):
    m = C.primal_grid(L, order)
    x = C.expand(m)
    a, b = E.Engine(0), E.Engine(0)
    try:
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            a.upload(m); a.set_reparametrization(mode)
            b.upload(x); b.set_reparametrization(mode)
            assert set(a.plan.schedule_classes(0, mode)) == {"diff"}
            ra, rb = a.readout(), b.readout()
            for it in range(2):
                a.compute_pass_and_primal(it); b.compute_pass_and_primal(it)            # the rounding pass
                assert np.array_equal(a.download_primal(), b.download_primal()), (mode, it)
                assert np.array_equal(a.download_duals(), b.download_duals()), (mode, it)
                assert a.check_primal_consistency() == b.check_primal_consistency()
                ca, cb = a.evaluate_primal(), b.evaluate_primal()
                assert ca == cb and np.isfinite(ca), (ca, cb)
                for direction in (0, 1):
                    for refine in (0, 1):
                        va, vb = a.decode_primal(direction, refine), b.decode_primal(direction, refine)
                        assert va == vb, (mode, it, direction, refine, va, vb)
                        assert np.array_equal(a.download_primal(), b.download_primal())
                        assert a.evaluate_primal() == b.evaluate_primal()
                ba, bb = ra.beliefs(), rb.beliefs()
                assert not np.any(np.isnan(ba)) and np.array_equal(ba, bb), (mode, it)
                a.compute_pass(1); b.compute_pass(1)
            ra.close(); rb.close()
        # against the oracle once: the rounding pass on the expansion is the reference's
        o = Oracle(x); o.set_reparametrization(M.REPAM_ANISOTROPIC)
        a.upload(m); a.set_reparametrization(M.REPAM_ANISOTROPIC)
        a.compute_pass_and_primal(0); o.ComputePassAndPrimal(0)
        assert np.array_equal(a.download_primal(), o.primal())
        c, co = a.evaluate_primal(), o.EvaluatePrimal()
        assert (c == co) if np.isinf(co) else abs(c - co) <= 1e-9 * max(1.0, abs(co)), (c, co)
    finally:
        a.close(); b.close()


# ---- new costs on the planned model -------------------------------------------------------------------------------------------
def _after(e, mode=M.REPAM_ANISOTROPIC, n=2):
    e.compute_pass(n)
    return e.download_duals(), e.lower_bound(), e.factor_lower_bounds()


def _fresh(model, mode=M.REPAM_ANISOTROPIC, n=2):
    e = E.Engine(0)
    try:
        e.upload(model); e.set_reparametrization(mode)
        return _after(e, mode, n)
    finally:
        e.close()


def _same(got, want):
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("source", ["host", "device"])
def test_set_constants_with_new_scales_and_shifts(source):
    m = C.recost_grid()
    fs = np.random.default_rng(8).permutation(np.flatnonzero(m.f_kind == SHIFT))[:20].astype(np.int32)
    rows = C.shift_rows(m, fs, 5)
    e = E.Engine(0)
    try:
        e.upload(m); e.set_reparametrization(M.REPAM_ANISOTROPIC)
        e.compute_pass(1)
        built, plan = e.schedules_built(), e.L.lpmp_engine_plan(e.h)
        duals = e.download_duals()
        if source == "device":
            import torch
            t = torch.from_numpy(np.pad(rows, ((0, 0), (0, 3)))).to("cuda:0")
            e.set_constants(fs, src_dev=t.data_ptr(), src_stride=5)
        else:
            e.set_constants(fs, rows)
        want_model = C.with_duals(C.with_rows(m, fs, rows), duals)
        _same(_after(e), _fresh(want_model))
        # the constants the cells are gathered from got the rows too: a warm upload_costs of NOTHING new keeps them
        assert e.schedules_built() == built and e.L.lpmp_engine_plan(e.h) == plan
    finally:
        e.close()


def test_upload_costs_cold_and_warm_and_a_new_pool():
    m = C.recost_grid()
    fs = np.flatnonzero(m.f_kind == SHIFT).astype(np.int32)
    m2 = C.with_rows(m, fs, C.shift_rows(m, fs, 6))
    e = E.Engine(0)
    try:
        e.upload(m); e.set_reparametrization(M.REPAM_ANISOTROPIC)
        e.compute_pass(1)
        built, plan = e.schedules_built(), e.L.lpmp_engine_plan(e.h)
        e.upload_costs(const=m2.const_data, duals=m2.dual_data)                  # cold
        _same(_after(e), _fresh(m2))
        duals = e.download_duals()
        e.upload_costs(const=m.const_data)                                       # warm: the first model's numbers on these duals
        _same(_after(e), _fresh(C.with_duals(m, duals)))
        # listed constants, then a warm upload of the array that holds them: the same state either way
        sub, rows = fs[::3], C.shift_rows(m, fs[::3], 7)
        m3 = C.with_rows(m, sub, rows)
        duals = e.download_duals()
        e.set_constants(sub, rows)
        e.upload_costs(const=m3.const_data)
        _same(_after(e), _fresh(C.with_duals(m3, duals)))
        # new VALUES for the pool
        duals = e.download_duals()
        sh = 0.125 + np.random.default_rng(2).uniform(0, 1, m.sh_data.shape[0])
        e.upload_shared_pool(sh)
        _same(_after(e), _fresh(C.with_duals(m3.with_pool(sh), duals)))
        assert e.schedules_built() == built and e.L.lpmp_engine_plan(e.h) == plan
        assert e.plan.diff_band_info(0, M.REPAM_ANISOTROPIC)["band_launches"] == 0
    finally:
        e.close()


def test_lp_set_factor_cost_sends_exactly_the_changed_factors():
    from lp_mp_amd import lp as LPM
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.diff_shift_pairwise_factor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    rng = np.random.default_rng(4)
    n, L = 8, 12

    def build(costs):
        lp = LPM.LP(LPM.FMC("SRMP", [U, P], [ML, MR]))
        t = lp.add_diff_table(M.truncated_linear_compact(0.25, 1.0)[0])
        u = [lp.add_factor(U, un[v]) for v in range(n)]
        p = []
        for v in range(n - 1):
            p.append(lp.add_factor(P, L, L, t, *costs[v]))
            lp.add_message(ML, u[v], p[-1]); lp.add_message(MR, u[v + 1], p[-1])
            lp.AddFactorRelation(u[v], p[-1]); lp.AddFactorRelation(p[-1], u[v + 1])
        return lp, p
    un = rng.uniform(0, 1, (n, L))
    old = [(float(rng.uniform(0.5, 2)), int(rng.integers(-3, 12))) for _ in range(n - 1)]
    new = list(old)
    new[2] = (0.75, old[2][1] + 2); new[5] = (old[5][0], -1)                     # a scale and a shift; a shift alone
    lp, p = build(old)
    e = lp._ready()
    e.set_reparametrization(M.REPAM_ANISOTROPIC)
    e.compute_pass(1)
    duals = e.download_duals()
    sent = []
    real = e.set_constants
    e.set_constants = lambda fs, rows, **kw: (sent.append((list(fs), np.array(rows))), real(fs, rows, **kw))[1]
    for v in (2, 5):
        lp.set_factor_cost(p[v], L, L, 0, *new[v])
    lp.upload_costs(warm=True)
    assert len(sent) == 1 and sent[0][0] == [p[2], p[5]], sent
    assert np.array_equal(sent[0][1], np.array([new[2], new[5]], np.float64))
    got = _after(e)
    lp2, _ = build(new)
    _same(got, _fresh(C.with_duals(lp2.flat_model(), duals)))


# ---- a seeded randomised family -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(C.N_FUZZ // C.FUZZ_BLOCK))
def test_random_models(block):
    """100 models: random graphs mixing DIFF_SHIFT with DIFF, SHARED, DENSE and POTTS, `left` / `right` / `full` schedules, a
    random weight mode and send rule each"""
    eng = E.Engine(0)
    try:
        for seed in range(C.FUZZ_BLOCK * block, C.FUZZ_BLOCK * (block + 1)):
            m, mode, rtype = C.fuzz_case(seed)
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
