"""The banded form of shifted difference-indexed factors on the device (sweep_diff_shift_band_kernel).  The yardstick is the CPU
oracle on the dense expansion (``C.expand(m)``) on identical duals.  Duals: ``np.array_equal``.  Lower bounds, bit for bit in the two
forms the engine has them:
- recomputed from the duals (``invalidate_lower_bounds()``: min_a (m1[a] + min_b (T[a, b] + m2[b])), the oracle's expression): the
  per-factor bounds ``np.array_equal`` to the oracle's, and ``lower_bound()`` equal to the bit with those bounds added in the order
  the engine adds them (``C.lower_bound_as_summed``: the oracle adds by factor type, the engine a block tree);
- tracked by the sweep kernels (a pairwise factor's bound is min_x (m_s'[x] + q[x]) from the receiving side: the same number in
  another association, so it differs from the oracle's by roundings for EVERY kernel class — 8.9e-16 on the first model of this
  file, on the banded and on the full kernel alike): equal to the bit between the banded engine and the full-kernel engine, whose
  kernel is the parent's instruction for instruction, and within the project's 1e-12 per factor / 1e-5 relative of the oracle.

Every model runs on two engines: one as it comes — every launch of a banded model runs the new kernel: with timing on,
``shift_band_launches == launches > 0`` — and one planned under LPMP_NO_DIFF_BAND=1, which runs sweep_diff_shift_kernel
(``shift_band_launches == 0``).  Both must equal the oracle."""
import contextlib
import os

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from oracle.binding import Oracle

import diff_shift_band_cases as C
import diff_shift_cases as DS

pytestmark = pytest.mark.gpu

LB_RTOL = 1e-5
FLB_ATOL = 1e-12
ANISO, UNIFORM = M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM
FORMS = ("banded", "full")


@pytest.fixture(scope="module")
def engines():
    es = {k: E.Engine(0) for k in FORMS}
    yield es
    for e in es.values():
        e.close()


@contextlib.contextmanager
def _no_band(on):
    """LPMP_NO_DIFF_BAND is read when a plan is made (Engine.upload)"""
    old = os.environ.get("LPMP_NO_DIFF_BAND")
    if on:
        os.environ["LPMP_NO_DIFF_BAND"] = "1"
    else:
        os.environ.pop("LPMP_NO_DIFF_BAND", None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("LPMP_NO_DIFF_BAND", None)
        else:
            os.environ["LPMP_NO_DIFF_BAND"] = old


def _upload(e, form, m, mode, rtype=M.RTYPE_SHARED, **kw):
    with _no_band(form == "full"):
        e.upload(m, **kw)
    e.set_reparametrization_type(rtype)
    e.set_reparametrization(mode)
    e.enable_kernel_timing(True); e.reset_kernel_timing()


def _planned(e, form, mode, banded=True, only_diff=True):
    """asserted BEFORE anything runs: the class, and the kernel of every launch with a DIFF_SHIFT factor"""
    for d in (0, 1):
        if only_diff:
            assert set(e.plan.schedule_classes(d, mode)) == {"diff"}, e.plan.schedule_classes(d, mode)
        i = e.plan.diff_shift_band_info(d, mode)
        assert i["shift_launches"] > 0
        assert i["shift_band_launches"] == (i["shift_launches"] if banded and form == "banded" else 0), (form, i)
        assert e.plan.diff_band_info(d, mode)["band_launches"] == 0


def _counters(e, form, banded=True, what=""):
    """the counters of the timed launches since the last reset, then a reset"""
    kt = e.kernel_timing()["diff"]
    e.reset_kernel_timing()
    assert kt["kernel"] == "sweep_diff_shift_kernel" and kt["band_launches"] == 0 and kt["shift_launches"] == kt["launches"] > 0, (what, kt)
    if banded and form == "banded":
        assert kt["shift_band_launches"] == kt["launches"] > 0, (what, form, kt)
    else:
        assert kt["shift_band_launches"] == 0, (what, form, kt)
    return kt


class _Ref:
    """what the oracle holds at one point: duals, per-factor bounds, its total"""

    def __init__(self, o, m):
        self.d = o.duals().copy()
        self.flb = np.array([o.factor_lower_bound(f) for f in range(m.n_factors)])
        self.lb = o.LowerBound()
        self.summed = C.lower_bound_as_summed(self.flb, m.constant)


def _same(e, r, what=""):
    """returns the tracked bounds (per factor, total) for the comparison between the two engines"""
    d = e.download_duals()
    assert not np.any(np.isnan(d)), what
    assert np.array_equal(d, r.d), (what, float(np.max(np.abs(d - r.d))))
    flb, lb = e.factor_lower_bounds(), e.lower_bound()
    print("tracked bounds %r: max |flb - oracle| = %.3g, lb - oracle = %.3g" % (what, float(np.max(np.abs(flb - r.flb))), lb - r.lb))
    assert np.max(np.abs(flb - r.flb)) <= FLB_ATOL, what
    assert np.isfinite(lb) and abs(lb - r.lb) <= LB_RTOL * max(1.0, abs(r.lb)), (what, lb, r.lb)
    e.invalidate_lower_bounds()
    flb2 = e.factor_lower_bounds()
    assert np.array_equal(flb2, r.flb), (what, float(np.max(np.abs(flb2 - r.flb))))
    lb2 = e.lower_bound()
    assert lb2 == r.summed, (what, lb2, r.summed)
    return flb, lb


def _steps(m, mode, rtype=M.RTYPE_SHARED):
    """the oracle at upload, after a forward pass, a backward pass and compute_pass(3): computed once for both engines"""
    o = Oracle(C.expand(m)); o.set_reparametrization_type(rtype); o.set_reparametrization(mode)
    out = [("upload", _Ref(o, m))]
    for name, run in (("forward", o.ComputeForwardPass), ("backward", o.ComputeBackwardPass), ("three passes", lambda: o.ComputePass(3))):
        run()
        out.append((name, _Ref(o, m)))
    return out


def _check(engines, m, modes=C.MODES, rtype=M.RTYPE_SHARED, banded=True, only_diff=True):
    assert C.banded(m) == banded
    for mode in modes:
        steps = _steps(m, mode, rtype)
        tracked = {}
        for form in FORMS:
            e = engines[form]
            _upload(e, form, m, mode, rtype)
            _planned(e, form, mode, banded, only_diff)
            for name, ref in steps:
                if name == "forward":
                    e.forward_pass()
                elif name == "backward":
                    e.backward_pass()
                elif name == "three passes":
                    e.compute_pass(3)
                tracked[form, name] = _same(e, ref, (form, mode, name))
            _counters(e, form, banded, (form, mode))
            e.enable_kernel_timing(False)
        for name, _ in steps:        # the bounds the kernels track: the banded form against the full kernel, bit for bit
            assert np.array_equal(tracked["banded", name][0], tracked["full", name][0]) and tracked["banded", name][1] == tracked["full", name][1], (mode, name)
    engines["banded"].set_reparametrization_type(M.RTYPE_SHARED); engines["full"].set_reparametrization_type(M.RTYPE_SHARED)


# ---- the kernel: every LDS size class, the four / two wave edge, every placement of the band -----------------------------------------
@pytest.mark.parametrize("L", C.GRID_LABELS)
@pytest.mark.parametrize("order", C.ORDERS)
def test_grids_every_lds_size_class_every_placement(engines, L, order):
    """the named vectors (n = 1, n = 2, constant, an empty band with unequal tails, unequal and equal tails, +inf tails, -0.0 against
    +0.0 ends, the widest admitted band), every edge at a named placement of its band: centred, clipped at either end, wholly left,
    wholly right, shift 0, d1 - 1, +-(n + L), +-2^30"""
    _check(engines, C.label_grid(L, order))


def test_rectangular_chains_both_sides(engines):
    for kw in C.RECT_CHAINS:
        _check(engines, C.rect_chain(**kw), modes=(ANISO, UNIFORM))


def test_plain_diff_and_shifted_peers_in_one_record(engines):
    _check(engines, C.mixed_kinds_grid(), modes=(ANISO, UNIFORM))


def test_rule_edge_and_one_unbanded_vector_run_the_full_kernel(engines):
    _check(engines, C.rule_grid(40, 0), modes=(ANISO,))
    _check(engines, C.rule_grid(40, 1), modes=(ANISO,), banded=False)
    _check(engines, C.one_unbanded_grid(), modes=(ANISO,), banded=False)


@pytest.mark.parametrize("rtype", C.RTYPES)
@pytest.mark.parametrize("L", [40, 130])
def test_send_rules_and_a_rounding_sweep(engines, rtype, L):
    """send rules shared and residual; then compute_pass_and_primal: duals and labels against the oracle"""
    m = C.label_grid(L, "colour_major", compute_primal=True)
    _check(engines, m, modes=(ANISO, UNIFORM), rtype=rtype)
    x = C.expand(m)
    for mode in (ANISO, UNIFORM):
        o = Oracle(x); o.set_reparametrization_type(rtype); o.set_reparametrization(mode)
        o.ComputePass(1); o.ComputePassAndPrimal(0)
        for form in FORMS:
            e = engines[form]
            _upload(e, form, m, mode, rtype)
            e.compute_pass(1); e.compute_pass_and_primal(0)
            assert np.array_equal(e.download_duals(), o.duals()), (form, mode)
            assert np.array_equal(e.download_primal(), o.primal()), (form, mode)
            c, co = e.evaluate_primal(), o.EvaluatePrimal()
            assert (c == co) if np.isinf(co) else abs(c - co) <= 1e-9 * max(1.0, abs(co)), (c, co)
            _counters(e, form, True, (form, mode, "rounding"))
            e.enable_kernel_timing(False)
            e.set_reparametrization_type(M.RTYPE_SHARED)


# ---- new costs on the planned model: the counters follow the pool, never a shift -------------------------------------------------------
def _pass_equals_oracle(e, m, mode, what):
    """one pass of the engine from where it is against the oracle on ``m`` with the engine's duals"""
    d = e.download_duals()
    o = Oracle(DS.with_duals(C.expand(m), d)); o.set_reparametrization(mode)
    e.compute_pass(1); o.ComputePass(1)
    _same(e, _Ref(o, m), what)


def test_move_windows_moves_the_bands(engines):
    """windows of 64 labels on the compact truncated-linear vector (9 entries); moves of up to +-150 labels push bands out of the
    window on either side"""
    m, _ = C.window_chain()
    assert C.banded(m)
    rng = np.random.default_rng(3)
    for form in FORMS:
        e = engines[form]
        _upload(e, form, m, ANISO)
        _planned(e, form, ANISO)
        e.compute_pass(2)
        _counters(e, form, True, "before the move")
        cur = m
        ws = e.window_set()
        for delta in (rng.integers(-3, 4, ws.n), rng.integers(-150, 151, ws.n), rng.integers(-40, 41, ws.n)):
            d = e.download_duals()
            ws.move(delta)
            cur, d2 = M.move_windows(cur, d, None, delta)
            assert np.array_equal(e.download_duals(), d2)
            _pass_equals_oracle(e, cur, ANISO, (form, "after a move"))
            _counters(e, form, True, "after a move")
        ws.close()
        e.enable_kernel_timing(False)


def test_set_constants_with_new_scales_and_shifts(engines):
    m = C.compact_grid()
    factors = np.flatnonzero(m.f_kind == M.F_PAIRWISE_DIFF_SHIFT)[::2].astype(np.int32)
    for form in FORMS:
        e = engines[form]
        _upload(e, form, m, ANISO)
        e.compute_pass(2)
        _counters(e, form, True, "before")
        cur = m
        for seed in (1, 2):
            rows = DS.shift_rows(cur, factors, seed)
            if seed == 2:
                rows[::3, 1] = np.where(np.arange(rows[::3].shape[0]) % 2 == 0, 2.0 ** 30, -2.0 ** 30)
            e.set_constants(factors, rows)
            cur = DS.with_rows(cur, factors, rows)
            _planned(e, form, ANISO)
            _pass_equals_oracle(e, cur, ANISO, (form, "set_constants", seed))
            _counters(e, form, True, "after set_constants")
        e.enable_kernel_timing(False)


def test_upload_shared_pool_unbands_and_rebands_after_graph_replays(engines):
    """row-major: more launches per sweep than the threshold of graph replay, and the passes before the first swap have been replayed
    from captured graphs; a graph that kept the other kernel would run it on the new pool"""
    m, banded_a, unbanded, banded_b = C.repool_grid(order="row_major")
    for form in FORMS:
        e = engines[form]
        _upload(e, form, m, ANISO)
        assert e.plan.schedule_info(0, ANISO)["n_launches"] > 8
        e.compute_pass(3); e.forward_pass(); e.backward_pass(); e.compute_pass(2)
        _counters(e, form, True, "before")
        for vectors, want in ((unbanded, False), (banded_b, True), (banded_a, True), (unbanded, False)):
            cur = C.with_pool(m, vectors)
            assert C.banded(cur) == want
            e.upload_shared_pool(cur.sh_data)
            _planned(e, form, ANISO, banded=want)
            assert e.plan.diff_shift_bands() == {t: M.diff_band(v) for t, v in enumerate(vectors)}
            _pass_equals_oracle(e, cur, ANISO, (form, "pool", want))
            e.compute_pass(2)
            _counters(e, form, want, ("after the pool", want))
        e.enable_kernel_timing(False)


# ---- far offsets ---------------------------------------------------------------------------------------------------------------
def test_shifted_banded_sweep_behind_2_31_elements():
    """one model of this file behind 2^31 elements of padding, in the borrowed buffers of tests/test_far_offsets_gpu.py"""
    import test_far_offsets_gpu as FO
    bufs = FO._buffers("P31")
    try:
        m = C.label_grid(65, "colour_major")
        with FO.Far(bufs, m, ANISO) as x:
            x.classes(only={"diff"})
            for d in (0, 1):
                i = x.e.plan.diff_shift_band_info(d, ANISO)
                assert i["shift_band_launches"] == i["shift_launches"] > 0
            kt = x.standard("diff shift banded")
            assert kt["diff"]["shift_band_launches"] == kt["diff"]["launches"] > 0 and kt["diff"]["kernel"] == "sweep_diff_shift_kernel", kt
    finally:
        FO._release(bufs)
