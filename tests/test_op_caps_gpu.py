"""The packed sweep kernels at their op-count caps and the device at its size limits, against the oracle (the models:
tests/op_cap_cases.py; why these inputs can fail: tests/test_op_caps_host.py).  A record with exactly cap ops fills the LDS slab of its
lane group to the last 16-byte piece and the next group's slab starts right behind it: an off-by-one in a slab size, in the indirect
branch of the packet load, in the chunked receive loop or in the prefetch of the first sends shows as wrong duals of a NEIGHBOURING
record, only at these op counts.  The yardstick is ``_check`` of tests/test_engine_gpu.py, restated with the tighter bounds of the
later test files: the oracle on identical input, duals ``np.array_equal`` after every call, the bound within 1e-9 relative, the
factors' bounds within 1e-12 — and the class split is asserted BEFORE anything runs, so that no other class can stand in."""
import numpy as np
import pytest

from lp_mp_amd import model as M
from lp_mp_amd import engine as E
from lp_mp_amd.multi_gpu import _cat_rows
from oracle.binding import Oracle

import op_cap_cases as OC

pytestmark = pytest.mark.gpu

LB_RTOL = 1e-9
FLB_ATOL = 1e-12
ANISO, UNIFORM = M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM
LPMP_ERR_UNSUPPORTED = -2                         # include/lpmp_engine.h
# (the last call is timed per kernel class: the records every class RAN must be those of the split, _run)
CALLS = (("pass", 1), ("pass", 1), ("pass", 1), ("forward", 0), ("pass", 2), ("backward", 0))


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def _call(x, what, n):
    oracle = isinstance(x, Oracle)
    if what == "pass":
        x.ComputePass(n) if oracle else x.compute_pass(n)
    elif what == "forward":
        x.ComputeForwardPass() if oracle else x.forward_pass()
    else:
        x.ComputeBackwardPass() if oracle else x.backward_pass()


_REFERENCE = {}


def _reference(key, build, mode, rtype=0, calls=CALLS):
    """the oracle on a model over ``calls``, computed once per (model, mode, send rule) and left unchanged: duals and bound after every
    call, the factors' bounds at the end"""
    key = (key, mode, rtype, calls)
    if key not in _REFERENCE:
        m = build()
        o = Oracle(OC.oracle_model(m))
        o.set_reparametrization_type(rtype); o.set_reparametrization(mode)
        steps = []
        for what, n in calls:
            _call(o, what, n)
            d = o.duals().copy(); d.setflags(write=False)
            steps.append((d, o.LowerBound()))
        flb = np.array([o.factor_lower_bound(f) for f in range(m.n_factors)]); flb.setflags(write=False)
        _REFERENCE[key] = (steps, flb)
    return _REFERENCE[key]


def _same(e, duals, bound, what):
    d = e.download_duals()
    assert np.array_equal(d, duals), (what, float(np.max(np.abs(d - duals))), int(np.sum(d != duals)))
    lb = e.lower_bound()
    assert abs(lb - bound) <= LB_RTOL * max(1.0, abs(bound)), (what, lb, bound)


def _expected_split(c, m, p, d, mode):
    s = OC.sweep(p, d, mode)
    return OC.expected_pairwise_split(c, m, s) if c.kind == "pairwise" else OC.split(OC.expected_record_classes(c, m, s)[1])


def _upload(e, c, m, mode, precision="f64", nt=0):
    """upload, set the mode, and assert the class split of both sweeps before anything runs"""
    e.upload(m, table_precision=precision)
    assert e.table_precision() == precision and e.L.lpmp_streaming_access(e.h) == nt
    e.set_reparametrization(mode)
    p = e.plan
    for d in OC.DIRECTIONS:
        assert p.schedule_classes(d, mode) == _expected_split(c, m, p, d, mode), (c.name, d, mode)


def _run(e, c, mode, rtype=0, precision="f64", nt=0, calls=CALLS):
    m = c.model()
    f32 = precision != "f64"
    steps, flb = _reference((c.name, f32), (lambda: m.with_f32_tables()) if f32 else (lambda: m), mode, rtype, calls)
    e.set_reparametrization_type(rtype)
    try:
        _upload(e, c, m, mode, precision, nt)
        for k, ((what, n), (duals, bound)) in enumerate(zip(calls, steps)):
            timed = k == len(calls) - 1 and what == "backward"
            if timed:
                e.enable_kernel_timing(True); e.reset_kernel_timing()
            _call(e, what, n)
            if timed:
                kt = e.kernel_timing(); e.reset_kernel_timing(); e.enable_kernel_timing(False)
                assert {k_: v["factors"] for k_, v in kt.items()} == _expected_split(c, m, e.plan, M.BACKWARD, mode), (c.name, mode, kt)
            _same(e, duals, bound, (c.name, mode, rtype, precision, k, what, n))
        assert np.max(np.abs(e.factor_lower_bounds() - flb)) <= FLB_ATOL, (c.name, mode)
    finally:
        e.enable_kernel_timing(False)
        e.set_reparametrization_type(0)


def test_the_census_is_complete():
    assert OC.census_gaps(OC.census(OC.cases(), E.Plan)) == []


# ---- every hub_side and star case in all four weight modes --------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in OC.family("hub_side") + OC.family("star")])
def test_records_at_the_caps_equal_the_oracle(eng, name):
    c = OC.case(name)
    for mode in OC.MODES:
        _run(eng, c, mode)


@pytest.mark.parametrize("name", [c.name for c in OC.family("pw_dup")])
def test_updated_pairwise_factors_at_their_cap(eng, name):
    """3 + 3 ops = PW_MAX_OPS stay on the packed pairwise class in the uniform modes, 4 + 4 run on the generic kernel"""
    c = OC.case(name)
    for mode in OC.MODES:
        _run(eng, c, mode)


# ---- crosses: the at-cap cases of the exact classes and of one run-time-dims class (dense_v8) ------------------------------------
CROSS = [c for c in OC.family("hub_side") + OC.family("star") if c.at_cap and (c.exact or c.cls == "dense_v8")]
CROSS_MODES = (ANISO, UNIFORM)


@pytest.mark.parametrize("name", [c.name for c in CROSS])
def test_cross_residual_send_rule(eng, name):
    for mode in CROSS_MODES:
        _run(eng, OC.case(name), mode, rtype=1)


@pytest.mark.parametrize("name", [c.name for c in CROSS])
def test_cross_non_temporal_kernels(eng, name, monkeypatch):
    """LPMP_NT=1 (read at every upload) forces the non-temporal instantiations of the exact kernels, as the nt_eng fixture of
    tests/test_engine_gpu.py does"""
    monkeypatch.setenv("LPMP_NT", "1")
    for mode in CROSS_MODES:
        _run(eng, OC.case(name), mode, nt=1)


@pytest.mark.parametrize("name", [c.name for c in CROSS if c.kind == "dense"])
def test_cross_float_tables(name):
    """table_precision="f32_round" against the oracle on the rounded model (an engine of its own: the request outlives an upload)"""
    e = E.Engine(0)
    try:
        for mode in CROSS_MODES:
            _run(e, OC.case(name), mode, precision="f32_round")
    finally:
        e.close()


@pytest.mark.parametrize("name", [c.name for c in CROSS])
def test_cross_rounding_passes(eng, name):
    c = OC.case(name)
    m = c.model(compute_primal=True)
    for mode in CROSS_MODES:
        o = Oracle(m); o.set_reparametrization(mode)
        eng.upload(m, table_precision="f64"); eng.set_reparametrization(mode)
        p = eng.plan
        for d in OC.DIRECTIONS:          # (COMPUTE_PRIMAL keeps every record: the models of the list have none without ops)
            assert p.schedule_classes(d, mode) == _expected_split(c, m, p, d, mode), (name, d, mode)
        for it in (1, 2):
            o.ComputePassAndPrimal(it); eng.compute_pass_and_primal(it)
            assert np.array_equal(eng.download_primal(), o.primal()), (name, mode, it)
            cost, want = eng.evaluate_primal(), o.EvaluatePrimal()
            assert abs(cost - want) <= 1e-9 * max(1.0, abs(want)), (name, mode, it, cost, want)
            _same(eng, o.duals(), o.LowerBound(), (name, mode, it))


@pytest.mark.parametrize("name", [c.name for c in CROSS])
def test_cross_fused_custom_schedule(eng, name):
    """forward rows + backward rows as ONE fused schedule (lpmp_schedule_create_fused), run twice"""
    c = OC.case(name)
    m = c.model()
    for mode in CROSS_MODES:
        o = Oracle(m); o.set_reparametrization(mode)
        _upload(eng, c, m, mode)
        rows = []
        for d in OC.DIRECTIONS:
            oo, om = o.omega(d, mode); mo, mk = o.mask(d, mode)
            rows.append((o.update_order(d), oo, om, mo, mk))
        cat = _cat_rows(*rows)
        sid = eng.schedule_create(*cat, fuse=True)
        info = eng.schedule_info(sid)
        assert info["n_receives"] == int(cat[4].sum()) and info["n_sends"] == int((cat[2] != 0).sum()), (name, mode)
        for k in range(2):
            eng.schedule_run(sid); o.compute_pass_custom(*cat)
            _same(eng, o.duals(), o.LowerBound(), (name, mode, k))
        eng.schedule_destroy(sid)


# ---- the chain executor in the indirect form ------------------------------------------------------------------------------------
BANDED_CALLS = (("pass", 1), ("pass", 3), ("forward", 0), ("backward", 0))


@pytest.mark.parametrize("name", [c.name for c in OC.family("banded") + OC.family("mixed_chain")])
def test_banded_chains_with_every_record_at_the_cap(name, monkeypatch):
    """one chain launch per sweep whose full records hold 2 k > PK_MAX_OPS ops (``ln.stride < 0`` with ``CHAIN = true``), and the same
    passes one launch per level (LPMP_NO_CHAIN=1), as in test_chain_executor_deep_schedules: both against the oracle, bit for bit.
    The mixed chain: packet levels and indirect levels in ONE launch, one of them at the cap."""
    c = OC.case(name)
    m = c.model()
    engines = []
    for env in ("0", "1"):
        monkeypatch.setenv("LPMP_NO_CHAIN", env)
        engines.append(E.Engine(0))
    monkeypatch.delenv("LPMP_NO_CHAIN")
    try:
        for mode in OC.MODES:
            steps, flb = _reference((name, False), lambda: m, mode, 0, BANDED_CALLS)
            for e in engines:
                _upload(e, c, m, mode)
            if mode in OC.ANISO_MODES:
                for d in OC.DIRECTIONS:
                    ci = engines[0].plan.chain_info(d, mode)
                    assert ci["n_chains"] == 1 and ci["n_plain_launches"] == 0 and ci["mailbox_rows"] == 0, (name, mode, d, ci)
            for k, ((what, n), (duals, bound)) in enumerate(zip(BANDED_CALLS, steps)):
                for j, e in enumerate(engines):
                    _call(e, what, n)
                    _same(e, duals, bound, (name, mode, "no chain" if j else "chain", k, what, n))
            for e in engines:
                assert np.max(np.abs(e.factor_lower_bounds() - flb)) <= FLB_ATOL, (name, mode)
        # the residual rule adds to a sent vector once more
        calls = (("forward", 0), ("pass", 2))
        steps, _ = _reference((name, False), lambda: m, ANISO, 1, calls)
        for j, e in enumerate(engines):
            e.set_reparametrization_type(1)
            _upload(e, c, m, ANISO)
            for (what, n), (duals, bound) in zip(calls, steps):
                _call(e, what, n)
                _same(e, duals, bound, (name, "residual", "no chain" if j else "chain", what, n))
    finally:
        for e in engines:
            e.close()


# ---- the limits ---------------------------------------------------------------------------------------------------------------------
def test_a_hub_with_32767_active_receives_and_sends(eng):
    """int16_t n_recv / n_send at their largest value: REPAM_UNIFORM gives the hub 32767 receives AND 32767 sends, REPAM_ANISOTROPIC
    16383 + 16384; the hub alone runs on the streaming class (its level's launch follows it: run-time dims)"""
    name = "star 2 labels %d spokes" % OC.MAX_ACTIVE
    m = OC.LIMITS[name]()
    calls = (("pass", 1), ("pass", 1))
    for mode in (UNIFORM, ANISO):
        steps, flb = _reference((name, False), lambda: m, mode, 0, calls)
        eng.upload(m, table_precision="f64"); eng.set_reparametrization(mode)
        p = eng.plan
        s = OC.sweep(p, M.FORWARD, mode)
        assert (s.n_recv.max(), s.n_send.max()) == ((OC.MAX_ACTIVE, OC.MAX_ACTIVE) if mode == UNIFORM else (OC.MAX_ACTIVE // 2, OC.MAX_ACTIVE // 2 + 1))
        for d in OC.DIRECTIONS:
            assert p.schedule_classes(d, mode) == {"dense_v4": OC.MAX_ACTIVE, "dense_big": 1}, (d, mode)
        for k, ((what, n), (duals, bound)) in enumerate(zip(calls, steps)):
            _call(eng, what, n)
            _same(eng, duals, bound, (name, mode, k))
        assert np.max(np.abs(eng.factor_lower_bounds() - flb)) <= FLB_ATOL, mode


def test_a_hub_with_32768_active_messages_is_refused_and_the_engine_goes_on():
    """lpmp_set_reparametrization builds the directional schedules: LPMP_ERR_UNSUPPORTED (include/lpmp_engine.h, size limits), and the
    same engine runs the next model"""
    m = OC.LIMITS["star 2 labels %d spokes" % (OC.MAX_ACTIVE + 1)]()
    e = E.Engine(0)
    try:
        e.upload(m)
        with pytest.raises(E.EngineError) as err:
            e.set_reparametrization(UNIFORM)
        assert err.value.code == LPMP_ERR_UNSUPPORTED and "32767" in str(err.value), str(err.value)
        c = OC.case("star dense 16 labels 64 spokes hub middle")
        _run(e, c, UNIFORM)
        _run(e, c, ANISO)
    finally:
        e.close()


@pytest.mark.parametrize("name", [n for n in OC.LIMITS if "spokes" not in n] + ["star 40 labels 300 spokes"])
@pytest.mark.parametrize("precision", ["f64", "f32_round"])
def test_streaming_class_at_its_label_limit(name, precision):
    """dense_big at 320 .. 512 labels (LDS sized by ceil(max_dim / 64)), on rectangular tables with a side of 512, and with a receive
    loop of 300 ops; anisotropic and uniform, double and float tables, one rounding pass at the end"""
    m = OC.LIMITS[name](True)
    x = m.with_f32_tables() if precision != "f64" else m
    n_rec = int(np.sum(m.f_kind == M.F_VECTOR))
    e = E.Engine(0)
    try:
        for mode in (ANISO, UNIFORM):
            o = Oracle(x); o.set_reparametrization(mode)
            e.upload(m, table_precision=precision); e.set_reparametrization(mode)
            assert e.table_precision() == precision
            for d in OC.DIRECTIONS:
                assert e.plan.schedule_classes(d, mode) == {"dense_big": n_rec}, (name, d, mode)
            for k in range(2):
                o.ComputePass(1); e.compute_pass(1)
                _same(e, o.duals(), o.LowerBound(), (name, precision, mode, k))
            flb = np.array([o.factor_lower_bound(f) for f in range(m.n_factors)])
            assert np.max(np.abs(e.factor_lower_bounds() - flb)) <= FLB_ATOL, (name, precision, mode)
            o.ComputePassAndPrimal(1); e.compute_pass_and_primal(1)
            assert np.array_equal(e.download_primal(), o.primal()), (name, precision, mode)
            cost, want = e.evaluate_primal(), o.EvaluatePrimal()
            assert abs(cost - want) <= 1e-9 * max(1.0, abs(want)), (name, precision, mode, cost, want)
            _same(e, o.duals(), o.LowerBound(), (name, precision, mode, "rounding"))
    finally:
        e.close()
