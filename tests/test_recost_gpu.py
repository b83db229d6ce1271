"""New costs on the plan that is already there: lpmp_upload_costs / lpmp_set_vectors / lpmp_zero_pairwise_duals (include/lpmp_engine.h).

Procedure everywhere: upload A, set the weights, run passes (so that schedules, chain caches and tracked bounds exist), hand the engine
the costs of B — the same structure, another seed — and run again.  Yardsticks: the unchanged CPU oracle on B (on its expansion for
SHARED / DIFF factors, on ``B.with_f32_tables()`` for float tables) and a FRESH engine that uploads B the ordinary way and receives the
same calls.  Duals ``np.array_equal`` to both after the last pass; the lower bound within 1e-5 relative of the oracle's after every
pass and ``==`` the fresh engine's (both recompute every factor from all-stale with the same code); per-factor bounds within 1e-12.
And nothing is planned: the plan handle and ``schedules_built()`` do not change, across the call and across the passes after it.
The one case in which the count may move is not asserted on: a WARM start while passes ran ahead settles by replaying the passes the
caller asked for, and the joined launch of that pass count is built if the engine never ran it (include/lpmp_engine.h)."""
import contextlib
import dataclasses

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import lp as LPM
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import recost_cases as C

pytestmark = pytest.mark.gpu

LB_RTOL = 1e-5
FLB_ATOL = 1e-12
ANISO, UNIFORM = M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -2, -4


def _same(e, f, o, what=""):
    d = e.download_duals()
    assert not np.any(np.isnan(d)), what
    assert np.array_equal(d, f.download_duals()), what
    assert np.array_equal(d, o.duals()), (what, float(np.max(np.abs(d - o.duals()))))
    flb = e.factor_lower_bounds()
    assert np.max(np.abs(flb - f.factor_lower_bounds())) <= FLB_ATOL, what
    n = min(flb.shape[0], 1500)
    assert np.max(np.abs(flb[:n] - np.array([o.factor_lower_bound(k) for k in range(n)]))) <= FLB_ATOL, what


def _passes(e, f, o, n=3, what=""):
    for k in range(n):
        e.compute_pass(1); f.compute_pass(1); o.ComputePass(1)
        lb, lbf, lbo = e.lower_bound(), f.lower_bound(), o.LowerBound()
        print(what, "pass", k, "lower bound", lb, "fresh engine", lbf, "oracle", lbo)
        assert lb == lbf, (what, k)
        assert abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (what, k, lb, lbo)


@contextlib.contextmanager
def recosted(A, B, mode=ANISO, upload_kw=None, oracle_of=C.oracle_model, recost=None, warm_up=3):
    """(e, f, o): e ran ``warm_up`` passes on A and received B's costs; f is a fresh engine on B; o the oracle on B"""
    kw = dict(upload_kw or {})
    e, f = E.Engine(0), E.Engine(0)
    try:
        e.upload(A, **kw); e.set_reparametrization(mode)
        for _ in range(warm_up):
            e.compute_pass(1); e.lower_bound()
        handle, built = e.plan.h, e.schedules_built()
        assert built > 0
        if recost is None:
            e.upload_costs(const=B.const_data, duals=B.dual_data)
        else:
            recost(e)
        assert e.plan.h == handle and e.schedules_built() == built
        f.upload(B, **kw); f.set_reparametrization(mode)
        assert f.schedules_built() > 0                 # what a fresh upload plans again
        o = Oracle(oracle_of(B)); o.set_reparametrization(mode)
        e.planned = (handle, built)
        yield e, f, o
        assert e.plan.h == handle and e.schedules_built() == built
    finally:
        e.close(); f.close()


def _procedure(A, B, mode=ANISO, what="", **kw):
    with recosted(A, B, mode, **kw) as (e, f, o):
        _passes(e, f, o, 3, what)
        _same(e, f, o, what)
        assert e.schedules_built() == e.planned[1]
        # the directional schedules are the cached ones, too
        for x in (e, f):
            x.forward_pass(); x.backward_pass()
        o.ComputeForwardPass(); o.ComputeBackwardPass()
        _same(e, f, o, what + " directional")


# ---- every storage path and kernel family ---------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["colour_major", "row_major"])
@pytest.mark.parametrize("L", [4, 13, 32, 40])
def test_engine_owned_f64(L, order):
    A = C.grid(7, 6, L, order)
    B = C.recost(A, 1000 + L)
    for mode in (ANISO, UNIFORM):
        _procedure(A, B, mode, "f64 L=%d %s" % (L, order))


def test_potts():
    A = C.grid(7, 6, 8, "colour_major", "potts")
    _procedure(A, C.recost(A, 21), what="potts")


def test_shared_tables_all_scales_change():
    A = C.shared_grid()
    B = C.recost(A, 22)
    assert np.all(A.const_data != B.const_data) and np.array_equal(A.sh_data, B.sh_data)
    with recosted(A, B) as (e, f, o):
        assert list(e.plan.schedule_classes(0, ANISO)) == ["shared32"]
        _passes(e, f, o, 3, "shared")
        _same(e, f, o, "shared")


@pytest.mark.parametrize("L,banded", [(40, True), (13, False)])
def test_diff_vectors(L, banded):
    A = C.diff_grid(L, banded)
    B = C.recost(A, 23)
    with recosted(A, B) as (e, f, o):
        assert list(e.plan.schedule_classes(0, ANISO)) == ["diff"]
        assert (e.plan.diff_band_info(0, ANISO)["band_launches"] > 0) == banded
        _passes(e, f, o, 3, "diff")
        _same(e, f, o, "diff")
        # the banded kernel ran on A's plan and runs on B: the band words in front of the pool entries were not touched
        e.enable_kernel_timing(True); e.reset_kernel_timing()
        e.compute_pass(1); f.compute_pass(1); o.ComputePass(1)
        kt = e.kernel_timing(); e.enable_kernel_timing(False)
        assert (kt["diff"]["band_launches"] > 0) == banded, kt
        _same(e, f, o, "diff, timed pass")


def test_rows_layout():
    A = C.rows_graph()
    B = C.recost(A, 24)
    with recosted(A, B, upload_kw=dict(rows_layout=True)) as (e, f, o):
        assert e.rows_layout and f.rows_layout
        _passes(e, f, o, 3, "rows")
        _same(e, f, o, "rows")
    # warm start under the rows layout: the rows hold the newer messages when the call comes
    e, f = E.Engine(0), E.Engine(0)
    try:
        e.upload(A, rows_layout=True); e.set_reparametrization(ANISO); e.compute_pass(3)
        e.upload_costs(const=B.const_data)
        oa = Oracle(A); oa.set_reparametrization(ANISO); oa.ComputePass(3)
        d3 = oa.duals()
        assert np.array_equal(e.download_duals(), d3)
        warm = dataclasses.replace(B, dual_data=d3, _keep=[])
        f.upload(warm, rows_layout=True); f.set_reparametrization(ANISO)
        o = Oracle(warm); o.set_reparametrization(ANISO)
        _passes(e, f, o, 2, "rows warm")
        _same(e, f, o, "rows warm")
    finally:
        e.close(); f.close()


def test_labeling_list_model():
    A = C.c5_small()
    _procedure(A, C.recost(A, 25), what="c5")


def test_deep_schedule_as_a_chain_with_the_mailbox(monkeypatch):
    monkeypatch.delenv("LPMP_NO_MAILBOX", raising=False); monkeypatch.delenv("LPMP_NO_CHAIN", raising=False)
    A = C.mailbox_grid()
    ci = E.Plan(A).chain_info(M.FORWARD, ANISO)
    assert ci["n_chains"] == 1 and ci["mailbox_rows"] > 0
    _procedure(A, C.recost(A, 26), what="mailbox chain")


def test_joined_pass_launch_keeps_its_ticket_templates(monkeypatch):
    # LPMP_ROT_BANDS, the switch tests/test_speculation_gpu.py forces the JOINED-pass launch with, not the LPMP_BAND_* pair of
    # tests/test_engine_gpu.py:460: that pair bands the chain of a SINGLE sweep or pass and leaves the cache of joined-pass ticket
    # templates (chain_cache_bytes) empty on a model of this size — the cache is what this test is about
    monkeypatch.setenv("LPMP_ROT_BANDS", "6")
    A = C.grid(40, 36, 32, "colour_major")
    B = C.recost(A, 27)
    e, f = E.Engine(0), E.Engine(0)
    try:
        e.upload(A); e.set_reparametrization(ANISO); e.compute_pass(4); e.lower_bound()
        cache, built, handle = e.chain_cache_bytes(), e.schedules_built(), e.plan.h
        assert cache > 0 and built > 0
        e.upload_costs(const=B.const_data, duals=B.dual_data)
        assert e.chain_cache_bytes() == cache and e.schedules_built() == built and e.plan.h == handle
        f.upload(B); f.set_reparametrization(ANISO)
        o = Oracle(B); o.set_reparametrization(ANISO)
        e.compute_pass(4); f.compute_pass(4); o.ComputePass(4)
        assert e.lower_bound() == f.lower_bound()
        _same(e, f, o, "joined passes")
        assert e.chain_cache_bytes() == cache and e.schedules_built() == built
    finally:
        e.close(); f.close()


# ---- borrowed device buffers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ["other tensors", "in place", "warm"])
def test_borrowed_buffers(way):
    import torch
    A = C.grid(7, 6, 13, "colour_major")
    B = C.recost(A, 31)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    const, dual = dev(A.const_data), dev(A.dual_data)
    torch.cuda.synchronize()
    e, f = E.Engine(0), E.Engine(0)
    try:
        e.upload(A, const_dev=const.data_ptr(), dual_dev=dual.data_ptr(), keep=(const, dual)); e.set_reparametrization(ANISO)
        for _ in range(3):
            e.compute_pass(1); e.lower_bound()
        handle, built = e.plan.h, e.schedules_built()
        e.synchronize()
        start = B
        if way == "other tensors":
            c2, d2 = dev(B.const_data), dev(B.dual_data)
            torch.cuda.synchronize()
            e.upload_costs(const_dev=c2.data_ptr(), dual_dev=d2.data_ptr())
            del c2, d2                                  # copied in: the engine still reads its first two tensors
            assert e.device_duals_ptr() == dual.data_ptr()
        elif way == "in place":
            const.copy_(torch.from_numpy(B.const_data)); dual.copy_(torch.from_numpy(B.dual_data))
            torch.cuda.synchronize()
            e.upload_costs(const_dev=const.data_ptr(), dual_dev=dual.data_ptr())
        else:
            before = e.download_duals()
            e.upload_costs(const=B.const_data)
            assert np.array_equal(e.download_duals(), before)
            assert np.array_equal(dual.cpu().numpy(), before)
            start = dataclasses.replace(B, dual_data=before, _keep=[])
        assert e.plan.h == handle and e.schedules_built() == built
        assert np.array_equal(const.cpu().numpy(), B.const_data)
        f.upload(start); f.set_reparametrization(ANISO)
        o = Oracle(start); o.set_reparametrization(ANISO)
        _passes(e, f, o, 3, way)
        _same(e, f, o, way)
        assert e.schedules_built() == built
    finally:
        e.close(); f.close()


# ---- float tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [13, 32])
def test_f32_strict_with_float_valued_costs(L):
    A = C.grid(7, 6, L, "colour_major").with_f32_tables()
    B = C.recost(A, 41, float_valued=True)
    with recosted(A, B, upload_kw=dict(table_precision="f32")) as (e, f, o):
        assert e.table_precision() == "f32"
        _passes(e, f, o, 3, "f32")
        _same(e, f, o, "f32")


def test_f32_round_with_arbitrary_costs():
    A = C.grid(7, 6, 13, "colour_major")
    B = C.recost(A, 42)
    assert np.any(B.const_data.astype(np.float32).astype(np.float64) != B.const_data)
    with recosted(A, B, upload_kw=dict(table_precision="f32_round"), oracle_of=lambda m: m.with_f32_tables()) as (e, f, o):
        _passes(e, f, o, 3, "f32_round")
        _same(e, f, o, "f32_round")


def test_f32_from_a_borrowed_buffer_and_from_device_data():
    """the two other storage paths of float tables: tables narrowed out of the caller's device buffer, and an engine whose compact
    constants came from host memory receiving device data (a mixed model: Potts cells are gathered, dense tables narrowed)"""
    import torch
    import f32_tables_cases as FC
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    A = FC.mixed_graph().with_f32_tables()
    B = C.recost(A, 43, float_valued=True)
    for borrowed in (True, False):
        e, f = E.Engine(0), E.Engine(0)
        try:
            ca, cb = dev(A.const_data), dev(B.const_data)
            torch.cuda.synchronize()
            if borrowed:
                e.upload(A, const_dev=ca.data_ptr(), keep=(ca,), table_precision="f32")
            else:
                e.upload(A, table_precision="f32")
            e.set_reparametrization(ANISO); e.compute_pass(2)
            built = e.schedules_built()
            e.upload_costs(const_dev=cb.data_ptr(), duals=B.dual_data)
            assert e.schedules_built() == built
            f.upload(B, table_precision="f32"); f.set_reparametrization(ANISO)
            o = Oracle(B); o.set_reparametrization(ANISO)
            _passes(e, f, o, 2, "f32 device data")
            _same(e, f, o, "f32 device data")
        finally:
            e.close(); f.close()


def test_f32_strict_refusal_leaves_the_constants_unspecified_until_good_costs_come():
    A = C.grid(7, 6, 13, "colour_major").with_f32_tables()
    B = C.recost(A, 44, float_valued=True)
    dense = np.flatnonzero(A.f_kind == M.F_PAIRWISE_DENSE)
    k = int(dense[5])
    bad = np.array(B.const_data, copy=True)
    bad[A.const_offsets()[k] + 3] = 0.1                  # not a float
    e, f = E.Engine(0), E.Engine(0)
    try:
        e.upload(A, table_precision="f32"); e.set_reparametrization(ANISO); e.compute_pass(2)
        handle, built = e.plan.h, e.schedules_built()
        with pytest.raises(E.EngineError, match=r"factor %d\b" % k) as ei:
            e.upload_costs(const=bad, duals=B.dual_data)
        assert ei.value.code == ERR_UNSUPPORTED
        for call in (lambda: e.compute_pass(1), e.lower_bound, e.forward_pass, e.factor_lower_bounds):
            with pytest.raises(E.EngineError) as ei:
                call()
            assert ei.value.code == ERR_STATE
        e.upload_costs(const=B.const_data, duals=B.dual_data)
        assert e.plan.h == handle and e.schedules_built() == built
        f.upload(B, table_precision="f32"); f.set_reparametrization(ANISO)
        o = Oracle(B); o.set_reparametrization(ANISO)
        _passes(e, f, o, 3, "after the refusal")
        _same(e, f, o, "after the refusal")
    finally:
        e.close(); f.close()


def test_call_order():
    e = E.Engine(0)
    try:
        e.model = C.grid(7, 6, 4)
        with pytest.raises(E.EngineError) as ei:
            e.upload_costs(const=e.model.const_data, duals=np.zeros(0))
        assert ei.value.code == ERR_STATE                # before the first upload
        e.upload(e.model)
        with pytest.raises(E.EngineError) as ei:
            e.upload_costs()
        assert ei.value.code == ERR_STATE                # neither half given
    finally:
        e.close()


# ---- passes that ran ahead ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", [False, True])
def test_passes_that_ran_ahead(warm, monkeypatch):
    monkeypatch.setenv("LPMP_ROT_BANDS", "6")
    A = C.grid(40, 36, 32, "colour_major")
    B = C.recost(A, 51)
    e, f, g = E.Engine(0), E.Engine(0), E.Engine(0)
    try:
        e.upload(A); e.set_reparametrization(ANISO); e.lower_bound()
        e.set_speculation(8)
        for _ in range(3):
            e.compute_pass(1)
        st = e.speculation_stats()
        assert st["batches"] >= 1 and st["passes_launched"] > st["passes_used"] == 3, st   # the device is ahead of the caller
        if warm:
            e.upload_costs(const=B.const_data)
            g.upload(A); g.set_reparametrization(ANISO); g.compute_pass(3)
            d3 = g.download_duals()
            assert np.array_equal(e.download_duals(), d3)          # the batch was settled: exactly 3 passes
            start = dataclasses.replace(B, dual_data=d3, _keep=[])
        else:
            e.upload_costs(const=B.const_data, duals=B.dual_data)
            assert e.speculation_stats()["rollbacks"] == st["rollbacks"]   # the batch was dropped, not replayed
            start = B
        # from here on both engines receive the same calls: a bound out of a batch's rows is a tracked one, the fresh engine's first
        # one is recomputed from the duals — the same three numbers added in another order (tests/test_speculation_gpu.py)
        e.set_speculation(0)
        f.upload(start); f.set_reparametrization(ANISO)
        o = Oracle(start); o.set_reparametrization(ANISO)
        _passes(e, f, o, 3, "ran ahead, warm" if warm else "ran ahead, cold")
        _same(e, f, o, "ran ahead")
    finally:
        e.close(); f.close(); g.close()


# ---- primal --------------------------------------------------------------------------------------------------------------------
def test_primal_labels_go_back_to_unset():
    A = C.grid(9, 8, 8, "colour_major", compute_primal=True)
    B = C.recost(A, 61)
    e = E.Engine(0)
    try:
        e.upload(A); e.set_reparametrization(ANISO); e.compute_pass_and_primal(0)
        assert np.isfinite(e.evaluate_primal())
        e.upload_costs(const=B.const_data, duals=B.dual_data)
        unset = np.stack([A.f_dim0, np.where(A.f_kind == M.F_VECTOR, 0, A.f_dim1)], 1).astype(np.int32)
        assert np.array_equal(e.download_primal(), unset)
        assert e.evaluate_primal() == np.inf
        e2 = E.Engine(0)
        try:
            e2.upload(B); e2.set_reparametrization(ANISO); e2.compute_pass_and_primal(1)
            e.compute_pass_and_primal(1)
            assert np.array_equal(e.download_primal(), e2.download_primal())
            assert e.evaluate_primal() == e2.evaluate_primal()
            assert np.array_equal(e.download_duals(), e2.download_duals())
        finally:
            e2.close()
        o2 = Oracle(B); o2.set_reparametrization(ANISO); o2.ComputePassAndPrimal(1)
        assert np.array_equal(e.download_primal(), o2.primal())
        assert abs(e.evaluate_primal() - o2.EvaluatePrimal()) <= 1e-9 * max(1.0, abs(o2.EvaluatePrimal()))
    finally:
        e.close()


# ---- custom schedules and halos ----------------------------------------------------------------------------------------------
def test_custom_schedules_and_halos_survive():
    import torch
    A = C.grid(9, 8, 8, "colour_major")
    B = C.recost(A, 71)
    o = Oracle(B); o.set_reparametrization(ANISO)
    oo, om = o.omega(0, ANISO); mo, mk = o.mask(0, ANISO)
    rows = (o.update_order(0), oo, om, mo, mk)
    off = A.dual_offsets()
    vec = np.flatnonzero(A.f_kind == M.F_VECTOR)[:7]
    e = E.Engine(0)
    try:
        e.upload(A); e.set_reparametrization(ANISO)
        sid = e.schedule_create(*rows)
        halo = e.halo_create(off[vec], A.f_dim0[vec], np.zeros(0, np.int64), np.zeros(0, np.int32))
        e.schedule_run(sid); e.compute_pass(1)
        built = e.schedules_built()
        e.upload_costs(const=B.const_data, duals=B.dual_data)
        buf = torch.zeros(e.halo_sizes(halo)[0], dtype=torch.float64, device="cuda")
        e.halo_pack(halo, buf.data_ptr()); e.synchronize(); torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), np.concatenate([B.dual_data[off[v]:off[v + 1]] for v in vec]))
        e.schedule_run(sid); o.compute_pass_custom(*rows)
        assert np.array_equal(e.download_duals(), o.duals())
        assert e.schedules_built() == built
        e.halo_destroy(halo)
    finally:
        e.close()


# ---- set_vectors ---------------------------------------------------------------------------------------------------------------
def _prime(e):
    """every per-factor bound recomputed from the duals: from here on no entry of the bound array is one a sweep kernel tracked (such
    an entry adds the same three numbers of a pairwise cost in another order and may differ from the recomputed one by an ulp)"""
    e.invalidate_lower_bounds()
    e.lower_bound()


def _stale_marks_are_right(e):
    """after _prime and the call under test: the bound equals, with ==, the same engine's after invalidate_lower_bounds() — the
    entries the call marked stale are recomputed, the others are the recomputed ones of _prime, and both sums run over the same array"""
    lb = e.lower_bound()
    e.invalidate_lower_bounds()
    full = e.lower_bound()
    print("after the call", lb, "recomputed", full)
    assert lb == full, (lb, full)


def _vector_engine(m, passes=1):
    e = E.Engine(0)
    e.upload(m); e.set_reparametrization(ANISO)
    if passes:
        e.compute_pass(passes)
    e.lower_bound()
    return e


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("wide", [False, True], ids=["stride=longest", "stride>longest"])
def test_set_vectors_replace_and_accumulate(device, wide):
    import torch
    m = C.vector_lengths_model()
    vec = np.flatnonzero(m.f_kind == M.F_VECTOR)
    assert sorted(m.f_dim0[vec]) == [1, 3, 63, 64, 65, 300]
    stride = 300 + (17 if wide else 0)
    rows = S.u01(len(vec) * stride, 81).reshape(len(vec), stride)
    e, f = _vector_engine(m), E.Engine(0)
    try:
        for accumulate in (False, True):
            for factors in ([int(vec[2])], [int(v) for v in vec[::-1]]):       # n = 1; all of them, not in factor order
                _prime(e)
                before = e.download_duals()
                src = rows[:len(factors)]
                if device:
                    t = torch.from_numpy(np.ascontiguousarray(src)).cuda(); torch.cuda.synchronize()
                    e.set_vectors(factors, src_dev=t.data_ptr(), src_stride=stride, accumulate=accumulate)
                else:
                    e.set_vectors(factors, src, accumulate=accumulate)
                want = C.scatter_rows(m, before, factors, src, accumulate)
                assert np.array_equal(e.download_duals(), want), (accumulate, factors)
                _stale_marks_are_right(e)
        want = e.download_duals()
        f.upload(dataclasses.replace(m, dual_data=want, _keep=[])); f.set_reparametrization(ANISO)
        e.compute_pass(2); f.compute_pass(2)
        assert np.array_equal(e.download_duals(), f.download_duals())
    finally:
        e.close(); f.close()


def test_set_vectors_many_workgroups_and_only_what_changed_is_recomputed():
    A = C.grid(40, 30, 5, "colour_major")
    vec = np.flatnonzero(A.f_kind == M.F_VECTOR)
    assert len(vec) == 1200
    rows = S.u01(len(vec) * 8, 82).reshape(len(vec), 8)                    # one [H W, Lmax] cost volume, Lmax > L
    e, f = _vector_engine(A), E.Engine(0)
    try:
        before = e.download_duals()
        e.set_vectors(vec, rows)
        want = C.scatter_rows(A, before, vec, rows)
        assert np.array_equal(e.download_duals(), want)
        f.upload(dataclasses.replace(A, dual_data=want, _keep=[])); f.set_reparametrization(ANISO)
        e.compute_pass(2); f.compute_pass(2)
        assert np.array_equal(e.download_duals(), f.download_duals())
        _prime(e)
        e.set_vectors(vec[[3, 500, 77, 1199, 640]], rows[:5], accumulate=True)
        lb = e.lower_bound()
        assert 0 < e.lower_bound_recomputed() < A.n_factors and e.lower_bound_recomputed() == 5
        e.invalidate_lower_bounds()
        assert lb == e.lower_bound() and e.lower_bound_recomputed() == A.n_factors
    finally:
        e.close(); f.close()


def test_set_vectors_refusals_leave_the_duals_alone():
    m = C.vector_lengths_model()
    vec = [int(v) for v in np.flatnonzero(m.f_kind == M.F_VECTOR)]
    pw = int(np.flatnonzero(m.f_kind != M.F_VECTOR)[0])
    long_one = int(vec[int(np.argmax(m.f_dim0[vec]))])
    rows = np.ones((4, 300))
    e = _vector_engine(m)
    try:
        before = e.download_duals()
        cases = [([vec[0], vec[1], vec[0]], rows, None, r"factor %d\b" % vec[0]),
                 ([vec[0], pw], rows, None, r"factor %d\b" % pw),
                 ([vec[0], m.n_factors], rows, None, r"%d\b" % m.n_factors),
                 ([vec[0], -1], rows, None, r"-1\b"),
                 ([vec[0], long_one], rows.reshape(-1), 299, r"factor %d\b" % long_one)]
        for factors, src, stride, pattern in cases:
            with pytest.raises(E.EngineError, match=pattern) as ei:
                e.set_vectors(factors, src, src_stride=stride)
            assert ei.value.code == ERR_INVALID
            assert np.array_equal(e.download_duals(), before)
    finally:
        e.close()


# ---- zero_pairwise_duals -------------------------------------------------------------------------------------------------------
ZERO_MODELS = {
    "dense": (lambda: C.grid(7, 6, 13, "colour_major"), {}),
    "potts": (lambda: C.grid(7, 6, 8, "colour_major", "potts"), {}),
    "shared": (C.shared_grid, {}),
    "diff": (lambda: C.diff_grid(40, True), {}),
    "rows": (C.rows_graph, dict(rows_layout=True)),
}


@pytest.mark.parametrize("name", list(ZERO_MODELS))
def test_zero_pairwise_duals(name):
    A = ZERO_MODELS[name][0]()
    kw = ZERO_MODELS[name][1]
    B = C.recost(A, 91)
    vm = C.vector_mask(A)
    off = A.dual_offsets()
    vec = np.flatnonzero(A.f_kind == M.F_VECTOR)
    e, f = E.Engine(0), E.Engine(0)
    try:
        e.upload(A, **kw); e.set_reparametrization(ANISO); e.compute_pass(2); e.lower_bound()
        before = e.download_duals()
        assert np.any(before[~vm] != 0.0)
        built = e.schedules_built()
        _prime(e)
        e.zero_pairwise_duals()
        d = e.download_duals()
        assert np.array_equal(d[vm], before[vm])                              # the vector factors are untouched
        assert np.all(d[~vm] == 0.0) and not np.any(np.signbit(d[~vm]))       # +0.0, including the sign bit
        _stale_marks_are_right(e)
        # with set_vectors(all, replace): the cold start from device data = upload_costs(duals = B's)
        L = int(A.f_dim0[vec].max())
        rows = np.zeros((len(vec), L))
        for i, v in enumerate(vec):
            rows[i, :A.f_dim0[v]] = B.dual_data[off[v]:off[v + 1]]
        e.set_vectors(vec, rows)
        f.upload(A, **kw); f.set_reparametrization(ANISO); f.compute_pass(2)
        f.upload_costs(duals=B.dual_data)
        assert np.array_equal(e.download_duals(), B.dual_data) and np.array_equal(f.download_duals(), B.dual_data)
        assert abs(e.lower_bound() - f.lower_bound()) <= 1e-12 * max(1.0, abs(f.lower_bound()))
        e.compute_pass(2); f.compute_pass(2)
        assert np.array_equal(e.download_duals(), f.download_duals())
        o = Oracle(C.oracle_model(dataclasses.replace(A, dual_data=B.dual_data, _keep=[]))); o.set_reparametrization(ANISO); o.ComputePass(2)
        assert np.array_equal(e.download_duals(), o.duals())
        assert e.schedules_built() == built
    finally:
        e.close(); f.close()


# ---- the warm start is the right problem -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense", "shared"])
def test_warm_start_is_the_reparametrised_problem_of_the_new_costs(name):
    A = ZERO_MODELS[name][0]()
    B = C.recost(A, 95)
    off = A.dual_offsets()
    vec = np.flatnonzero(A.f_kind == M.F_VECTOR)
    changed = vec[::3]
    L = int(A.f_dim0[vec].max())
    delta = S.u01(len(changed) * L, 96).reshape(len(changed), L) - 0.5
    e = E.Engine(0)
    try:
        e.upload(A); e.set_reparametrization(ANISO); e.compute_pass(3)
        d3 = e.download_duals()
        e.upload_costs(const=B.const_data)
        assert np.array_equal(e.download_duals(), d3)
        e.set_vectors(changed, delta, accumulate=True)
        start = dataclasses.replace(B, dual_data=C.scatter_rows(A, d3, changed, delta, accumulate=True), _keep=[])
        assert np.array_equal(e.download_duals(), start.dual_data)
        o = Oracle(C.oracle_model(start)); o.set_reparametrization(ANISO)
        assert abs(e.lower_bound() - o.LowerBound()) <= LB_RTOL * max(1.0, abs(o.LowerBound()))
        e.compute_pass(2); o.ComputePass(2)
        assert np.array_equal(e.download_duals(), o.duals())
        assert abs(e.lower_bound() - o.LowerBound()) <= LB_RTOL * max(1.0, abs(o.LowerBound()))
    finally:
        e.close()


# ---- LP mirror -----------------------------------------------------------------------------------------------------------------
def _quick_start(u1c, u2c, pc):
    """the README quick-start model"""
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.PairwiseSimplexFactor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    lp = LPM.LP(LPM.FMC("SRMP", [U, P], [ML, MR]))
    u1, u2 = lp.add_factor(U, u1c), lp.add_factor(U, u2c)
    p = lp.add_factor(P, 2, 2, pc)
    lp.add_message(ML, u1, p); lp.add_message(MR, u2, p)
    lp.AddFactorRelation(u1, p); lp.AddFactorRelation(p, u2)
    return lp, (u1, u2, p)


def _solve(lp):
    s = LPM.MpRoundingSolver(lp, LPM.StandardVisitor(maxIter=50))
    s.Solve()
    return s.lower_bound(), s.primal_cost(), np.array(s.solution_, copy=True)


def test_lp_mirror_upload_costs_equals_a_new_lp():
    lp, (u1, u2, p) = _quick_start([0.0, 1.0], [1.0, 0.0], [[0.0, 1.0], [1.0, 0.0]])
    assert _solve(lp)[:2] == (1.0, 1.0)
    built = lp._engine.schedules_built()
    lp.set_factor_cost(u1, [0.7, 0.1])
    lp.set_factor_cost(p, 2, 2, [[0.0, 0.3], [0.6, 0.0]])
    assert not lp._dirty
    lp.upload_costs()
    assert lp._engine.schedules_built() == built          # the plan of the first solve
    got = _solve(lp)
    new, _ = _quick_start([0.7, 0.1], [1.0, 0.0], [[0.0, 0.3], [0.6, 0.0]])
    want = _solve(new)
    assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2])
    assert np.array_equal(lp.duals(), new.duals())
    # warm: the messages stay, bit for bit; the changed unary receives new - old
    before = lp.duals()
    lp.set_factor_cost(u2, [0.25, 0.5])
    lp.set_factor_cost(p, 2, 2, [[0.0, 2.0], [2.0, 0.0]])
    lp.upload_costs(warm=True)
    after = lp.duals()
    assert np.array_equal(after[4:], before[4:]) and np.array_equal(after[:2], before[:2])
    assert np.array_equal(after[2:4], before[2:4] + (np.array([0.25, 0.5]) - np.array([1.0, 0.0])))
    assert lp._engine.schedules_built() == built
    with pytest.raises(RuntimeError):
        lp.set_factor_cost(u1, [0.0, 1.0, 2.0])
    with pytest.raises(RuntimeError):
        lp.set_factor_cost(p, 2, 3, np.zeros((2, 3)))
