"""Float storage of dense pairwise tables on the device (lpmp_set_table_precision; Engine.upload(table_precision=...)).  The
yardstick everywhere is ``Oracle(m.with_f32_tables())`` on identical duals with the tolerances of tests/test_engine_gpu.py: duals
``np.array_equal`` after the last pass, lower bound within 1e-5 relative after every pass, per-factor bounds within 1e-12.
Kernel classes are asserted before anything runs and kernel names with the values, so that no other path can stand in for the
f32 kernels; tests/test_f32_tables_host.py shows that the yardstick differs from the f64 model's result."""
import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from oracle.binding import Oracle

import f32_tables_cases as C

pytestmark = pytest.mark.gpu

LB_RTOL = 1e-5
FLB_ATOL = 1e-12
MODES = C.MODES


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


def _check(eng, m, mode, passes=3, classes=None, kernels=None, precision="f32", rtype=0, upload=None, within=None):
    """precision "f32": strict upload of the rounded model; "f32_round": the engine rounds the model as it is.
    classes: the kernel classes both sweeps must consist of (within: a set they must lie in); kernels: class -> prefix of the
    kernel name that ran"""
    x = m.with_f32_tables()
    o = Oracle(x)
    o.set_reparametrization_type(rtype); o.set_reparametrization(mode)
    if upload is not None:
        upload(eng)
    else:
        eng.upload(x if precision == "f32" else m, table_precision=precision, rows_layout=False)
    assert eng.table_precision() == precision
    eng.set_reparametrization_type(rtype); eng.set_reparametrization(mode)
    try:
        if classes is not None:
            for d in (0, 1):
                assert set(eng.plan.schedule_classes(d, mode)) == set(classes), (eng.plan.schedule_classes(d, mode), classes)
        if within is not None:
            for d in (0, 1):
                assert set(eng.plan.schedule_classes(d, mode)) <= set(within), (eng.plan.schedule_classes(d, mode), within)
        lb0, lbo0 = eng.lower_bound(), o.LowerBound()
        assert abs(lb0 - lbo0) <= LB_RTOL * max(1.0, abs(lbo0)), (lb0, lbo0)
        eng.enable_kernel_timing(True); eng.reset_kernel_timing()
        for _ in range(passes):
            o.ComputePass(1)
            eng.compute_pass(1)
            lb, lbo = eng.lower_bound(), o.LowerBound()
            assert np.isfinite(lb) and abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (lb, lbo)
        kt = eng.kernel_timing(); eng.enable_kernel_timing(False)
        for cls, prefix in (kernels or {}).items():
            assert kt[cls]["kernel"].startswith(prefix), kt
        for cls, v in kt.items():
            if cls.startswith(("dense", "pairwise")):
                assert "_f32_kernel" in v["kernel"], kt
        d, do = eng.download_duals(), o.duals()
        assert not np.any(np.isnan(d))
        assert np.array_equal(d, do), float(np.max(np.abs(d - do)))
        flb = eng.factor_lower_bounds()
        oflb = np.array([o.factor_lower_bound(f) for f in range(min(m.n_factors, 3000))])
        assert np.max(np.abs(flb[:oflb.shape[0]] - oflb)) <= FLB_ATOL
    finally:
        eng.enable_kernel_timing(False)
        eng.set_reparametrization_type(0)
    return o


# ---- 1. exact classes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 8, 16, 32])
@pytest.mark.parametrize("order", ["colour_major", "row_major"])
def test_exact_classes_both_access_policies(nt_eng, L, order):
    m = C.grid(7, 6, L, order)
    for mode in MODES:
        _check(nt_eng, m, mode, 3, classes={"dense%d" % L}, kernels={"dense%d" % L: "sweep_dense_pk_f32_kernel<%d, " % L})
        assert nt_eng.L.lpmp_streaming_access(nt_eng.h) == nt_eng.want_nt


# ---- 2. run-time dims ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 5, 13, 21])
def test_run_time_dims_grids(eng, L):
    W = 4 if L <= 4 else 8 if L <= 8 else 16 if L <= 16 else 32
    for order in ("colour_major", "row_major"):
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            _check(eng, C.grid(7, 6, L, order), mode, 3, classes={"dense_v%d" % W}, kernels={"dense_v%d" % W: "sweep_dense_pk_f32_kernel<%d, " % W})


def test_rectangular_tables_with_unaligned_rows(eng):
    m = C.rect_chain()
    for mode in MODES:
        _check(eng, m, mode, 3)
    assert all(c.startswith("dense_v") for c in eng.plan.schedule_classes(0, M.REPAM_ANISOTROPIC))


def test_random_graph_half_dense_half_potts(eng):
    m = C.mixed_graph()
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_DAMPED_UNIFORM):
        _check(eng, m, mode, 3)
    assert eng.plan.schedule_classes(0, M.REPAM_ANISOTROPIC).get("dense_v8", 0) > 0


# ---- 3. streaming class -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [33, 64, 65, 130, pytest.param(("residual", 65), id="65-residual"), pytest.param(("residual", 130), id="130-residual"),
                               pytest.param(("rect", (5, 130, 5, 130)), id="5x130-rect")])
def test_streaming_class(nt_eng, L):
    """(the cases with a name: the residual send rule on a 3 x 3 grid, and a chain of 5- and 130-label variables, whose tables are
    received as rows by one neighbour and as columns by the other — the parts of the wave-per-unary text the plain grids leave out)"""
    what, L = L if isinstance(L, tuple) else ("grid", L)
    m = C.rect_chain(L) if what == "rect" else C.grid(3, 3, L, "colour_major") if what == "residual" else C.grid(4, 3, L, "colour_major")
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_DAMPED_UNIFORM):
        _check(nt_eng, m, mode, 2, classes={"dense_big"}, kernels={"dense_big": "sweep_dense_big_f32_kernel<"},
               rtype=M.RTYPE_RESIDUAL if what == "residual" else 0)


# ---- 4. updated pairwise factors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", [M.SCHED_RIGHT, M.SCHED_FULL])
@pytest.mark.parametrize("L", [5, 16, 33, pytest.param(("potts", 5), id="5-potts"), pytest.param(("rect", (2, 3, 7, 12, 30)), id="rect")])
def test_updated_pairwise_factors(eng, sched, L):
    """(the cases with a name: Potts factors, and tables of unequal dims — the other two branches of the packed kernel's load)"""
    what, L = L if isinstance(L, tuple) else ("dense", L)
    m = (C.scheduled_grid(3, 3, 0, sched, seed=3, dims=L) if what == "rect" else C.scheduled_grid(3, 3, L, sched, seed=L, potts=True) if what == "potts"
         else C.scheduled_grid(6, 5, L, sched, seed=L))
    for mode in MODES:
        _check(eng, m, mode, 2)
    cls = eng.plan.schedule_classes(M.BACKWARD, M.REPAM_UNIFORM)
    if what != "dense":
        assert sum(v for k, v in cls.items() if k.startswith("pairwise")) > 0 and "generic" not in cls
    elif L <= 32:
        want = "pairwise%d" % (8 if L <= 8 else 16 if L <= 16 else 32)
        assert cls.get(want, 0) > 0 and "generic" not in cls
    else:
        assert cls.get("generic", 0) > 0      # tables beyond the packed width: the generic kernel reads them entry by entry


# ---- 5. send rules on the generic kernels ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rtype", [M.RTYPE_RESIDUAL, M.RTYPE_ADAPTIVE])
def test_send_rules_on_the_generic_kernels(rtype):
    m = C.scheduled_grid(5, 4, 8, M.SCHED_LEFT, seed=3, flags=M.MF_IMPROVEMENT if rtype == M.RTYPE_ADAPTIVE else 0)
    e = E.Engine(0)
    try:
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_DAMPED_UNIFORM):
            # (the adaptive rule lives in the generic kernels; the residual rule runs in the packed body too)
            o = _check(e, m, mode, 3, rtype=rtype, within={"generic", "small"} if rtype == M.RTYPE_ADAPTIVE else None)
            if rtype == M.RTYPE_ADAPTIVE and mode == M.REPAM_ANISOTROPIC:
                assert o.counters()[1] > 0            # improvements were computed from the tables
    finally:
        e.close()


# ---- 6. joined passes as one persistent launch ------------------------------------------------------------------------------
@pytest.mark.parametrize("L,H,W", [(32, 40, 36), (8, 60, 70)])
def test_joined_passes_as_one_blocked_chain_launch(L, H, W, monkeypatch):
    monkeypatch.setenv("LPMP_ROT_BANDS", "8"); monkeypatch.setenv("LPMP_ROT_LAG", "2"); monkeypatch.setenv("LPMP_ROT_DEPTH", "4")
    m = C.grid(H, W, L, "colour_major").with_f32_tables()
    o = Oracle(m); o.set_reparametrization(M.REPAM_ANISOTROPIC)
    e = E.Engine(0)
    try:
        e.upload(m, table_precision="f32"); e.set_reparametrization(M.REPAM_ANISOTROPIC)
        assert e.plan.pass_rotates(M.REPAM_ANISOTROPIC)
        for n in (1, 5, 2, 9):
            e.enable_kernel_timing(True)
            e.compute_pass(n); o.ComputePass(n)
            kt = e.kernel_timing(); e.reset_kernel_timing(); e.enable_kernel_timing(False)
            assert set(kt) == {"dense%d" % L}
            assert all(v["kernel"].startswith("chain_dense_pk_f32_kernel<%d, " % L) and v["chain_launches"] == 1 for v in kt.values()), kt
            assert np.array_equal(e.download_duals(), o.duals()), (n,)
            assert abs(e.lower_bound() - o.LowerBound()) <= 1e-9 * max(1.0, abs(o.LowerBound()))
    finally:
        e.close()


# ---- 7. deep chains ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [16, 32])
@pytest.mark.parametrize("mailbox", [True, False], ids=["mailbox", "flags"])
def test_deep_chains(L, mailbox, monkeypatch):
    monkeypatch.setenv("LPMP_CHAIN_ALL", "1")
    if not mailbox:
        monkeypatch.setenv("LPMP_NO_MAILBOX", "1")
    m = C.grid(12, 10, L, "row_major").with_f32_tables()
    o = Oracle(m)
    e = E.Engine(0)
    try:
        e.upload(m, table_precision="f32")
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_DAMPED_UNIFORM):
            o.set_reparametrization(mode); e.set_reparametrization(mode)
            info = e.plan.chain_info(M.FORWARD, mode)
            assert info["n_chains"] == 1 and (info["mailbox_rows"] > 0) == mailbox, info
            # (no kernel timing here: a timed sweep runs launch by launch.  The chain plan above is what an untimed sweep
            # executes, its launch picks the f32 chain kernel from the engine's flag, and the f64 kernel could not stand in:
            # it would read the float buffer as doubles)
            for n in (1, 3):
                o.ComputePass(n); e.compute_pass(n)
                assert np.array_equal(e.download_duals(), o.duals()), (mode, n)
                assert abs(e.lower_bound() - o.LowerBound()) <= LB_RTOL * max(1.0, abs(o.LowerBound()))
            o.ComputeForwardPass(); o.ComputeBackwardPass()
            e.forward_pass(); e.backward_pass()
            assert np.array_equal(e.download_duals(), o.duals())
    finally:
        e.close()


# ---- 8. rounding ------------------------------------------------------------------------------------------------------------
def test_rounding_labels_and_cost(eng):
    # (8 labels: a packed class; 65 and 130: the streaming class, whose label rule is the wave-per-unary kernels' shared one)
    for m in (C.grid(6, 5, 8, "colour_major", compute_primal=True).with_f32_tables(), C.grid(3, 3, 65, "colour_major", compute_primal=True).with_f32_tables(),
              C.grid(3, 3, 130, "colour_major", compute_primal=True).with_f32_tables()):
        _rounding_labels_and_cost(eng, m)


def _rounding_labels_and_cost(eng, m):
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        o = Oracle(m); o.set_reparametrization(mode)
        eng.upload(m, table_precision="f32"); eng.set_reparametrization(mode)
        for it in range(3):
            eng.compute_pass_and_primal(it); o.ComputePassAndPrimal(it)
            assert np.array_equal(eng.download_primal(), o.primal())
            assert np.array_equal(eng.download_duals(), o.duals())
            assert eng.check_primal_consistency() == o.CheckPrimalConsistency()
            c, co = eng.evaluate_primal(), o.EvaluatePrimal()
            assert (c == co) if np.isinf(co) else abs(c - co) <= 1e-9 * max(1.0, abs(co)), (c, co)
        assert np.isfinite(eng.evaluate_primal())


# ---- 9. hard constraints ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [8, 32])
def test_hard_constraints(eng, L):
    def forbid(const, off, L=L):
        rng = np.random.default_rng(L)                     # (a grid's constants are its tables only)
        for t in rng.choice(const.shape[0] // (L * L), size=max(1, const.shape[0] // (L * L) // 10), replace=False):
            idx = rng.choice(L * L, size=L, replace=False)
            const[t * L * L + idx] = np.inf
    m = C.with_tables(C.grid(7, 6, L), forbid)
    assert np.isinf(m.const_data).any()
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_DAMPED_UNIFORM):
        _check(eng, m, mode, 3, classes={"dense%d" % L})
        _check(eng, m, mode, 3, classes={"dense%d" % L}, precision="f32_round")


# ---- 10. narrowing contract -------------------------------------------------------------------------------------------------
def test_narrowing_contract(eng):
    m = C.grid(7, 6, 8)
    first = int(C.dense_factors(m)[0])
    with pytest.raises(E.EngineError) as ei:
        eng.upload(m, table_precision="f32")                # random doubles are not floats
    assert ei.value.code == -2 and ("factor %d " % first) in str(ei.value), str(ei.value)
    # rounding on the device == strict on the rounded model
    _check(eng, m, M.REPAM_ANISOTROPIC, 3, classes={"dense8"}, precision="f32_round")
    a = eng.download_duals()
    _check(eng, m, M.REPAM_ANISOTROPIC, 3, classes={"dense8"}, precision="f32")
    assert np.array_equal(a, eng.download_duals())
    # beyond float's range, below FLT_MIN: refused in both modes, the factor is named (the lowest one: two tables are spoilt)
    x = m.with_f32_tables()
    off = m.const_offsets()
    dense = C.dense_factors(m)
    for bad in (1e39, -1e39, 1e-40, -1e-40):
        def spoil(const, _, bad=bad):
            const[off[dense[5]] + 3] = bad
            const[off[dense[9]] + 1] = bad
        y = C.with_tables(x, spoil)
        for prec in ("f32", "f32_round"):
            with pytest.raises(E.EngineError) as ei:
                eng.upload(y, table_precision=prec)
            assert ei.value.code == -2 and ("factor %d " % int(dense[5])) in str(ei.value), str(ei.value)
    # zero and the smallest normal float pass
    ok = C.with_tables(x, lambda const, _: const.__setitem__(slice(int(off[dense[5]]), int(off[dense[5]]) + 2), [0.0, float(np.finfo(np.float32).tiny)]))
    eng.upload(ok, table_precision="f32")
    assert eng.table_precision() == "f32"


def test_default_engine_is_f64_and_runs_the_f64_kernel():
    e = E.Engine(0)
    try:
        m = C.grid(7, 6, 8)
        e.upload(m); e.set_reparametrization(M.REPAM_ANISOTROPIC)
        assert e.table_precision() == "f64"
        e.enable_kernel_timing(True); e.compute_pass(1)
        kt = e.kernel_timing(); e.enable_kernel_timing(False)
        assert kt["dense8"]["kernel"].startswith("sweep_dense_pk_kernel<"), kt
        o = Oracle(m); o.set_reparametrization(M.REPAM_ANISOTROPIC); o.ComputePass(1)
        assert np.array_equal(e.download_duals(), o.duals())
        # the mode belongs to the upload: back to f64 on the same engine
        e.upload(m.with_f32_tables(), table_precision="f32"); assert e.table_precision() == "f32"
        e.upload(m, table_precision="f64"); assert e.table_precision() == "f64"
        e.set_reparametrization(M.REPAM_ANISOTROPIC); e.compute_pass(1)
        assert np.array_equal(e.download_duals(), o.duals())
    finally:
        e.close()


# ---- 11. refused combination ------------------------------------------------------------------------------------------------
def test_rows_layout_is_refused():
    e = E.Engine(0)
    try:
        with pytest.raises(E.EngineError) as ei:
            e.upload(C.grid(7, 6, 8).with_f32_tables(), table_precision="f32", rows_layout=True)
        assert ei.value.code == -2 and "rows layout" in str(ei.value)
    finally:
        e.close()


# ---- 12. borrowed device buffer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [8, 13])
def test_tables_in_a_callers_device_buffer(eng, L):
    import torch
    m = C.mixed_graph() if L == 8 else C.grid(7, 6, L, "row_major")
    x = m.with_f32_tables()
    const = torch.from_numpy(x.const_data).to("cuda:0")
    before = const.clone()

    def upload(e):
        e.upload(x, const_dev=const.data_ptr(), keep=(const,), table_precision="f32")
    _check(eng, m, M.REPAM_ANISOTROPIC, 3, upload=upload)
    a = eng.download_duals()
    assert torch.equal(const, before)                       # the caller's buffer is read, never written
    _check(eng, m, M.REPAM_ANISOTROPIC, 3)
    assert np.array_equal(a, eng.download_duals())
    eng.upload(C.grid(3, 3, 4), table_precision="f64")      # (lets go of the borrowed buffer; the mode stays as set until it is set again)


# ---- 13. memory -------------------------------------------------------------------------------------------------------------
def test_device_memory_of_an_f32_model():
    """128 x 128 x 32: 266 MB of f64 tables, 21 MB of duals.  The f32 engine may take at most 0.65 of what the f64 engine takes
    (the sizes give 0.55; the schedules do not shrink) — which also fails if the f64 tables or the staging buffer stay resident"""
    import torch
    m = C.grid(128, 128, 32, "colour_major", seed=9).with_f32_tables()
    drop = {}
    for prec in ("f64", "f32"):
        e = E.Engine(0)
        try:
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            e.upload(m, table_precision=prec); e.set_reparametrization(M.REPAM_ANISOTROPIC)
            drop[prec] = free0 - torch.cuda.mem_get_info()[0]
        finally:
            e.close()
    print("device memory taken: f64 %d, f32 %d bytes, ratio %.3f" % (drop["f64"], drop["f32"], drop["f32"] / drop["f64"]))
    assert drop["f64"] >= 266e6 and drop["f32"] <= 0.65 * drop["f64"], drop


# ---- the solver surface -------------------------------------------------------------------------------------------------------
UAI_TEXT = """MARKOV
4
3 3 3 2
7
1 0
1 1
1 2
1 3
2 0 1
2 1 2
2 2 3
3 0.1 0.7 0.3
3 0.5 0.2 0.9
3 0.4 0.4 0.1
2 0.6 0.2
9 0.0 1.0 2.0 1.0 0.0 1.0 2.0 1.0 0.0
9 0.0 1.0 2.5 1.0 0.0 1.0 2.5 1.0 0.0
6 %s
"""


def test_solve_uai_and_lp_set_table_precision():
    """LP.set_table_precision / solve_uai(table_precision=...): the third pairwise table is not float-valued — strict refuses it,
    rounding equals the f64 solver on the text whose table holds the rounded values (unary costs stay doubles everywhere)"""
    from lp_mp_amd import uai
    vals = [0.3, 0.9, 0.8, 0.1, 0.5, 0.5]
    text = UAI_TEXT % " ".join(repr(v) for v in vals)
    rounded = UAI_TEXT % " ".join(repr(float(np.float32(v))) for v in vals)
    ref = uai.solve_uai(rounded, maxIter=60)
    for got in (uai.solve_uai(text, table_precision="f32_round", maxIter=60), uai.solve_uai(rounded, table_precision="f32", maxIter=60)):
        assert got[0] == ref[0] and got[1] == ref[1] and np.array_equal(got[2], ref[2]), (got, ref)
    with pytest.raises(E.EngineError) as ei:
        uai.solve_uai(text, table_precision="f32", maxIter=60)
    assert ei.value.code == -2 and "factor 6 " in str(ei.value), str(ei.value)     # 4 unaries, then the pairwise factors 4, 5, 6
    lp = uai.build_lp_from_uai(rounded)
    lp.set_table_precision("f32")
    lp.set_reparametrization("anisotropic")
    lp.ComputePass(0)
    assert lp._engine.table_precision() == "f32"
    with pytest.raises(RuntimeError):
        lp.set_table_precision("f64")                   # the model is on the device
