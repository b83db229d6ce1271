"""New pairwise parameters on the plan that is already there: lpmp_upload_shared_pool (pool VALUES) and lpmp_set_constants (the
constants of listed pairwise factors), include/lpmp_engine.h.

Procedure: upload A, run passes (schedules, captured graphs and tracked bounds exist), make the call, run on.  Yardsticks, as in
tests/test_recost_gpu.py: the unchanged CPU oracle on the expansion of the model that holds the new numbers (``with_f32_tables()``
first under the float modes) and a FRESH engine that uploads that model the ordinary way — both started from the duals the engine
under test holds at the call (neither call touches the duals).  Duals ``np.array_equal`` to both, ``lower_bound() ==`` the fresh
engine's, the bound within 1e-5 relative of the oracle's, per-factor bounds within 1e-12.  Around every call and across the passes
after it the plan handle and ``schedules_built()`` do not move."""
import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import lp as LPM
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import recost_cases as C
import repool_cases as R

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


def _engine(A, mode=ANISO, passes=3, directional=0, **kw):
    """A uploaded, ``passes`` passes and ``directional`` forward + backward sweeps run: every built-in schedule exists"""
    e = E.Engine(0)
    e.upload(A, **kw); e.set_reparametrization(mode)
    for _ in range(passes):
        e.compute_pass(1); e.lower_bound()
    for _ in range(directional):
        e.forward_pass(); e.backward_pass()
    assert e.schedules_built() > 0
    return e


def _run_on(e, B, mode=ANISO, what="", oracle_of=R.oracle_model, n=3, band=None, **kw):
    """the engine under test holds the numbers of model B since the call under test: n passes and one directional sweep each way
    beside a fresh engine and the oracle on B, all from e's duals.  band: the directional sweeps are timed and the banded launches of
    class diff are the plan's prediction"""
    handle, built = e.plan.h, e.schedules_built()
    start = R.with_duals(B, e.download_duals())
    f = E.Engine(0)
    try:
        f.upload(start, **kw); f.set_reparametrization(mode)
        o = Oracle(oracle_of(start)); o.set_reparametrization(mode)
        _passes(e, f, o, n, what)
        _same(e, f, o, what)
        if band is not None:
            e.enable_kernel_timing(True); e.reset_kernel_timing()
        for x in (e, f):
            x.forward_pass(); x.backward_pass()
        o.ComputeForwardPass(); o.ComputeBackwardPass()
        if band is not None:
            kt = e.kernel_timing(); e.enable_kernel_timing(False)
            want = [e.plan.diff_band_info(d, mode) for d in (0, 1)]
            print(what, "timed", kt["diff"], "plan", want)
            assert kt["diff"]["launches"] == sum(w["diff_launches"] for w in want)
            assert kt["diff"]["band_launches"] == sum(w["band_launches"] for w in want)
            assert (kt["diff"]["band_launches"] > 0) == band
        _same(e, f, o, what + " directional")
        assert e.plan.h == handle and e.schedules_built() == built
    finally:
        f.close()


def _swap(e, B, **kw):
    handle, built = e.plan.h, e.schedules_built()
    before = e.download_duals()
    e.upload_shared_pool(B.sh_data, **kw)
    assert e.plan.h == handle and e.schedules_built() == built
    assert np.array_equal(e.download_duals(), before)          # the duals are not touched


# ---- pool swaps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["colour_major", "row_major"])
def test_diff_pool_banded_other_width_unbanded_banded(order):
    """row-major: 12 launches per sweep — the directional and pass schedules have been replayed from their captured graphs before the
    first swap, and a graph that kept the other kernel choice would read band words that are not there (or ignore the band)"""
    L = 40
    A = R.diff_grid(L, order)
    e = _engine(A, passes=3, directional=2)
    try:
        assert list(e.plan.schedule_classes(0, ANISO)) == ["diff"]
        if order == "row_major":
            assert e.plan.schedule_info(0, ANISO)["n_launches"] > 8         # (the threshold of graph replay, engine.cpp run_schedule)
        assert e.plan.diff_band_info(0, ANISO)["band_launches"] > 0
        for name, st, banded in (("other width", R.BANDED_2, True), ("unbanded", R.UNBANDED, False), ("banded again", R.BANDED, True)):
            B = A.with_pool(R.tl(L, st))
            assert M.diff_band_is_banded(B.sh_data) == banded
            _swap(e, B)
            assert e.plan.diff_bands() == {0: M.diff_band(B.sh_data) + (banded,)}
            _run_on(e, B, what="diff %s %s" % (order, name), band=banded)
    finally:
        e.close()


@pytest.mark.parametrize("L", [8, 130])
def test_diff_pool_lds_size_classes(L):
    """L = 8: LDS size class 1; L = 130: three 64-blocks, the last ragged"""
    banded = M.truncated_linear(L, L, 0.2, 0.2) if L == 8 else R.tl(L, R.BANDED)
    full = 0.125 + S.u01(2 * L - 1, 31)
    assert M.diff_band_is_banded(banded) and not M.diff_band_is_banded(full)
    first, second = (banded, full) if L == 8 else (full, banded)
    A = S.grid_model(7, 6, L, pairwise="diff", order="colour_major", seed=5, diff_tables=first[None])
    e = _engine(A)
    try:
        B = A.with_pool(second)
        _swap(e, B)
        _run_on(e, B, what="diff L=%d" % L, band=(L != 8))
    finally:
        e.close()


@pytest.mark.parametrize("name,source", [("13x11x32", "host"), ("7x6x13", "host"), ("7x6x13", "device"), ("5x6x40 generic", "host")])
def test_shared_pool(name, source):
    """new values for both tables, one holding a +inf entry; scales are positive.  shared32 (exact), shared16 with run-time dims, and
    the generic class, which reads the pool through pw_cost.  A device-pointer source gives what the host source gives."""
    A = {"13x11x32": C.shared_grid, "7x6x13": lambda: R.shared_grid_small(13),
         "5x6x40 generic": lambda: S.grid_model(5, 6, 40, pairwise="shared", order="colour_major", seed=8, n_tables=2)}[name]()
    assert np.all(A.const_data > 0)
    cls = list(E.Plan(A).schedule_classes(0, ANISO))
    assert cls == {"13x11x32": ["shared32"], "7x6x13": ["shared16"], "5x6x40 generic": ["generic"]}[name], cls
    B = A.with_pool(R.pool_of(A, 41, inf_at=A.sh_data.shape[0] // 2 + 7))
    e = _engine(A)
    try:
        if source == "device":
            import torch
            t = torch.from_numpy(B.sh_data).cuda(); torch.cuda.synchronize()
            handle, built = e.plan.h, e.schedules_built()
            e.upload_shared_pool(sh_dev=t.data_ptr())
            assert e.plan.h == handle and e.schedules_built() == built
        else:
            _swap(e, B)
        _run_on(e, B, what="shared " + name)
    finally:
        e.close()


def test_pool_swap_beside_float_tables():
    """DENSE, Potts, SHARED and DIFF parts in one model under f32: the swap rewrites the pool and leaves the float tables alone"""
    import mixed_precision_cases as MP
    A = MP.float_valued(MP.m1())
    Ld, Ls = MP.LABELS["diff"], MP.LABELS["shared"]
    sh = np.concatenate([0.125 + S.u01(2 * Ls * Ls, 51), R.tl(Ld, R.UNBANDED), R.tl(Ld, R.BANDED_2)])   # the two vectors change roles
    assert sh.shape == A.sh_data.shape
    B = A.with_pool(sh)
    e = _engine(A, table_precision="f32")
    try:
        b0 = e.plan.diff_band_info(0, ANISO)
        assert 0 < b0["band_launches"] < b0["diff_launches"]
        _swap(e, B)
        b1 = e.plan.diff_band_info(0, ANISO)
        assert b1["diff_launches"] == b0["diff_launches"] and 0 < b1["band_launches"] < b1["diff_launches"]
        _run_on(e, B, what="mixed f32", oracle_of=MP.oracle_model, band=True, table_precision="f32")
    finally:
        e.close()


def test_pool_swap_settles_passes_that_ran_ahead():
    """set_speculation(4): whatever ran ahead of the caller is settled before the pool moves — the duals at the swap are those of
    exactly the passes asked for (an engine without speculation is the witness)"""
    A = C.shared_grid()
    B = A.with_pool(R.pool_of(A, 61))
    e, g = E.Engine(0), E.Engine(0)
    try:
        e.upload(A); e.set_reparametrization(ANISO); e.lower_bound()
        e.set_speculation(4)
        for _ in range(3):
            e.compute_pass(1)
        g.upload(A); g.set_reparametrization(ANISO); g.compute_pass(3)
        _swap(e, B)
        assert np.array_equal(e.download_duals(), g.download_duals())
        _run_on(e, B, what="ran ahead")
    finally:
        e.close(); g.close()


def test_pool_swap_makes_bounds_stale_and_the_primal_unset():
    L = 40
    A = S.grid_model(7, 6, L, pairwise="diff", order="colour_major", seed=5, diff_tables=R.tl(L, R.BANDED)[None], compute_primal=True)
    B = A.with_pool(R.tl(L, R.UNBANDED))
    e = E.Engine(0)
    try:
        e.upload(A); e.set_reparametrization(ANISO); e.compute_pass_and_primal(0); e.lower_bound()
        assert np.isfinite(e.evaluate_primal())
        e.compute_pass(1); e.lower_bound()
        _swap(e, B)
        assert e.evaluate_primal() == np.inf
        lb = e.lower_bound()
        assert e.lower_bound_recomputed() == A.n_factors
        o = Oracle(R.oracle_model(R.with_duals(B, e.download_duals())))
        assert abs(lb - o.LowerBound()) <= LB_RTOL * max(1.0, abs(o.LowerBound()))
        e.compute_pass_and_primal(1)
        assert np.isfinite(e.evaluate_primal())
    finally:
        e.close()


def test_pool_refusals_leave_the_old_model_running():
    L = 40
    A = R.diff_grid(L, "colour_major")
    bad = np.array(R.tl(L, R.UNBANDED), copy=True); bad[11] = np.nan
    e, f = E.Engine(0), E.Engine(0)
    try:
        with pytest.raises(E.EngineError) as ei:
            e.upload_shared_pool(bad)
        assert ei.value.code == ERR_STATE                         # before the first upload
        e.upload(A); e.set_reparametrization(ANISO); e.compute_pass(2); e.lower_bound()
        bands, built = e.plan.diff_bands(), e.schedules_built()
        with pytest.raises(E.EngineError, match=r"table 0\b.*NaN") as ei:
            e.upload_shared_pool(bad)
        assert ei.value.code == ERR_INVALID
        with pytest.raises(E.EngineError) as ei:
            e.upload_shared_pool(None)
        assert ei.value.code == ERR_INVALID
        assert e.plan.diff_bands() == bands and e.schedules_built() == built
        f.upload(A); f.set_reparametrization(ANISO); f.compute_pass(2)
        o = Oracle(R.oracle_model(A)); o.set_reparametrization(ANISO); o.ComputePass(2)
        _passes(e, f, o, 2, "after the refusals")
        _same(e, f, o, "after the refusals")
        # a model without a pool
        g = C.grid(7, 6, 4)
        e.upload(g)
        with pytest.raises(E.EngineError) as ei:
            e.upload_shared_pool(np.zeros(4))
        assert ei.value.code == ERR_INVALID
    finally:
        e.close(); f.close()


# ---- listed constants ----------------------------------------------------------------------------------------------------------
def _listed(A, e, seed, mode=ANISO, what="", device=False, pad=0, float_valued=False, oracle_of=R.oracle_model, kinds=None, n=3, **kw):
    """set_constants of about a third of the pairwise factors in shuffled order, then the procedure on the model with those rows"""
    fs = R.listed_subset(A, seed, kinds)
    rows = R.rows_for(A, fs, seed + 1, float_valued=float_valued, stride=int(A.const_sizes()[fs].max()) + pad)
    handle, built = e.plan.h, e.schedules_built()
    before = e.download_duals()
    if device:
        import torch
        t = torch.from_numpy(np.ascontiguousarray(rows)).cuda(); torch.cuda.synchronize()
        e.set_constants(fs, src_dev=t.data_ptr(), src_stride=rows.shape[1])
    else:
        e.set_constants(fs, rows)
    assert e.plan.h == handle and e.schedules_built() == built
    assert np.array_equal(e.download_duals(), before)
    B = R.with_rows(A, fs, rows)
    assert not np.array_equal(B.const_data, A.const_data)
    _run_on(e, B, mode, what, oracle_of=oracle_of, n=n, **kw)
    return fs, rows, B


@pytest.mark.parametrize("L,device", [(4, False), (13, False), (13, True), (32, False), (40, False), (40, True)])
def test_listed_dense_f64(L, device):
    """exact, run-time-dims and streaming classes, engine-owned buffers; a host source, and a device source whose stride exceeds the rows"""
    A = C.grid(7, 6, L)
    e = _engine(A)
    try:
        _listed(A, e, 100 + L, what="listed dense L=%d" % L, device=device, pad=5 if device else 0)
    finally:
        e.close()


def test_listed_dense_in_a_borrowed_buffer():
    import torch
    A = C.grid(7, 6, 13)
    const = torch.from_numpy(np.ascontiguousarray(A.const_data)).cuda(); torch.cuda.synchronize()
    e = _engine(A, const_dev=const.data_ptr(), keep=(const,))
    try:
        fs, rows, B = _listed(A, e, 120, what="borrowed")
        e.synchronize()
        assert np.array_equal(const.cpu().numpy(), B.const_data)              # the caller's buffer holds the new tables
    finally:
        e.close()


def test_listed_dense_under_the_rows_layout():
    A = C.rows_graph()
    e = _engine(A, rows_layout=True)
    try:
        assert e.rows_layout
        _listed(A, e, 130, what="rows", rows_layout=True)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["potts", "shared", "diff"])
def test_listed_scalars(name):
    """the Potts scalar; SHARED / DIFF scales: the cell's first word, and the scalar the cell is gathered from — a later
    upload_costs without constants keeps the scales, and one with the same packed array reproduces them"""
    A = {"potts": lambda: C.grid(7, 6, 8, "colour_major", "potts"), "shared": C.shared_grid, "diff": lambda: C.diff_grid(40, True)}[name]()
    e = _engine(A)
    try:
        fs, rows, B = _listed(A, e, 140, what="listed " + name)
        if name != "potts":
            d = e.download_duals()
            e.upload_costs(duals=d)                                           # no constants: the cells are not gathered again
            _run_on(e, B, what=name + " after upload_costs(duals)", n=1)
            e.upload_costs(const=B.const_data)                                # gathered again, from the same numbers
            _run_on(e, B, what=name + " after upload_costs(const)", n=1)
    finally:
        e.close()


def test_listed_mixed_kinds_compact_constants_f32():
    """f32 with constants from host memory (the compact buffer: Potts / SHARED / DIFF cells only, tables as floats): listed factors of
    all four kinds, float-valued rows: accepted and exact"""
    import mixed_precision_cases as MP
    A = MP.float_valued(MP.m1())
    e = _engine(A, table_precision="f32")
    try:
        fs, rows, B = _listed(A, e, 150, what="mixed compact f32", float_valued=True, oracle_of=MP.oracle_model, table_precision="f32")
        assert len(set(A.f_kind[fs])) == 4
    finally:
        e.close()


def test_listed_f32_round_with_arbitrary_doubles():
    A = C.grid(7, 6, 13)
    e = _engine(A, table_precision="f32_round")
    try:
        fs, rows, B = _listed(A, e, 160, what="f32_round", oracle_of=lambda m: m.with_f32_tables(), table_precision="f32_round")
        assert np.any(rows.astype(np.float32).astype(np.float64) != rows)
    finally:
        e.close()


def test_listed_f32_in_a_borrowed_buffer():
    """the float tables take the rows; the caller's doubles are not written for tables"""
    import torch
    A = C.grid(7, 6, 13).with_f32_tables()
    const = torch.from_numpy(np.ascontiguousarray(A.const_data)).cuda(); torch.cuda.synchronize()
    e = _engine(A, const_dev=const.data_ptr(), keep=(const,), table_precision="f32")
    try:
        _listed(A, e, 170, what="borrowed f32", float_valued=True, table_precision="f32")
        e.synchronize()
        assert np.array_equal(const.cpu().numpy(), A.const_data)
    finally:
        e.close()


def test_listed_f32_refusal_writes_nothing():
    """one entry of the k-th listed table is not a float: LPMP_ERR_UNSUPPORTED naming that factor, and the next passes equal the
    oracle on the OLD costs bit for bit — no table of the list was written, the constants are not marked unspecified"""
    A = C.grid(7, 6, 13).with_f32_tables()
    fs = R.listed_subset(A, 180)
    rows = R.rows_for(A, fs, 181, float_valued=True)
    k = 5
    rows[k, 7] = 0.1
    rows[len(fs) - 1, 3] = 0.3                                                 # a second one: the LOWEST factor index is named
    named = int(min(fs[k], fs[len(fs) - 1]))
    e, f = E.Engine(0), E.Engine(0)
    try:
        e.upload(A, table_precision="f32"); e.set_reparametrization(ANISO); e.compute_pass(2); e.lower_bound()
        built = e.schedules_built()
        with pytest.raises(E.EngineError, match=r"factor %d\b" % named) as ei:
            e.set_constants(fs, rows)
        assert ei.value.code == ERR_UNSUPPORTED
        f.upload(A, table_precision="f32"); f.set_reparametrization(ANISO); f.compute_pass(2)
        o = Oracle(A); o.set_reparametrization(ANISO); o.ComputePass(2)
        _passes(e, f, o, 2, "after the refusal")
        _same(e, f, o, "after the refusal")
        assert e.schedules_built() == built
    finally:
        e.close(); f.close()


def test_listed_refusals_and_the_empty_list():
    A = C.grid(7, 6, 13)
    pw = [int(x) for x in np.flatnonzero(A.f_kind != M.F_VECTOR)[:3]]
    vec = int(np.flatnonzero(A.f_kind == M.F_VECTOR)[0])
    rows = np.ones((4, 169))
    e, f = E.Engine(0), E.Engine(0)
    try:
        e.upload(A); e.set_reparametrization(ANISO); e.compute_pass(2); e.lower_bound()
        before = e.download_duals()
        cases = [([pw[0], A.n_factors], rows, None, r"%d\b" % A.n_factors), ([pw[0], -1], rows, None, r"-1\b"),
                 ([pw[0], vec], rows, None, r"factor %d\b" % vec),
                 ([pw[0], pw[1], pw[0]], rows, None, r"factor %d\b" % pw[0]),
                 ([pw[0], pw[2]], rows.reshape(-1), 168, r"factor %d\b" % pw[0])]
        for factors, src, stride, pattern in cases:
            with pytest.raises(E.EngineError, match=pattern) as ei:
                e.set_constants(factors, src, src_stride=stride)
            assert ei.value.code == ERR_INVALID
        e.lower_bound()
        e.set_constants([], np.zeros((0, 169)))                               # n == 0: a no-op after the checks
        e.lower_bound()
        assert e.lower_bound_recomputed() == 0
        assert np.array_equal(e.download_duals(), before)
        f.upload(A); f.set_reparametrization(ANISO); f.compute_pass(2)
        o = Oracle(A); o.set_reparametrization(ANISO); o.ComputePass(2)       # constants and duals unchanged: the old model runs on
        _passes(e, f, o, 2, "after the refusals")
        _same(e, f, o, "after the refusals")
    finally:
        e.close(); f.close()


def test_listed_bounds_only_what_changed_is_recomputed():
    A = C.grid(7, 6, 13, compute_primal=True)
    fs = R.listed_subset(A, 190)
    rows = R.rows_for(A, fs, 191)
    e = E.Engine(0)
    try:
        e.upload(A); e.set_reparametrization(ANISO); e.compute_pass_and_primal(0)
        assert np.isfinite(e.evaluate_primal())
        e.invalidate_lower_bounds(); e.lower_bound()                          # every bound recomputed, none stale
        e.set_constants(fs, rows)
        assert e.evaluate_primal() == np.inf                                  # the labels belong to the old costs
        lb = e.lower_bound()
        k = e.lower_bound_recomputed()
        print("listed", len(fs), "recomputed", k, "of", A.n_factors)
        assert len(fs) <= k <= A.n_factors
        e.invalidate_lower_bounds()
        assert lb == e.lower_bound()
        B = R.with_duals(R.with_rows(A, fs, rows), e.download_duals())
        o = Oracle(B)
        assert abs(lb - o.LowerBound()) <= LB_RTOL * max(1.0, abs(o.LowerBound()))
        flb = e.factor_lower_bounds()
        assert np.max(np.abs(flb - np.array([o.factor_lower_bound(i) for i in range(A.n_factors)]))) <= FLB_ATOL
    finally:
        e.close()


# ---- LP mirror -------------------------------------------------------------------------------------------------------------------
def _lp_grid(kind, D, tables, unaries, scales, H=3, W=4, L=5):
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.diff_pairwise_factor if kind == "diff" else LPM.PairwiseSimplexFactor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    lp = LPM.LP(LPM.FMC("grid", [U, P], [ML, MR]), speculation=0)
    td = lp.add_diff_table(D) if kind == "diff" else None
    u = [lp.add_factor(U, unaries[i]) for i in range(H * W)]
    a, b = S.grid_edges(H, W)
    p = []
    for k, (i, j) in enumerate(zip(a, b)):
        i, j = int(min(i, j)), int(max(i, j))
        f = lp.add_factor(P, td, L, L, scales[k]) if kind == "diff" else lp.add_factor(P, L, L, tables[k])
        lp.add_message(ML, u[i], f); lp.add_message(MR, u[j], f)
        lp.AddFactorRelation(u[i], f); lp.AddFactorRelation(f, u[j])
        p.append(f)
    return lp, td, u, p


@pytest.mark.parametrize("kind", ["diff", "dense"])
def test_lp_mirror_warm_update_equals_a_new_lp_from_the_same_duals(kind):
    H, W, L = 3, 4, 5
    nE = len(S.grid_edges(H, W)[0])
    un = S.u01(H * W * L, 201).reshape(H * W, L)
    D0, D1 = M.truncated_linear(L, L, 0.5, 0.5), M.truncated_linear(L, L, 0.1, 0.3)
    tabs = S.u01(nE * L * L, 202).reshape(nE, L, L)
    sc = 0.5 + S.u01(nE, 203)
    lp, td, u, p = _lp_grid(kind, D0, tabs, un, sc)
    lp.set_reparametrization("anisotropic")
    for it in range(3):
        lp.ComputePass(it)
    built, handle = lp._engine.schedules_built(), lp._engine.plan.h
    duals = lp.duals()
    tabs2, sc2 = tabs.copy(), sc.copy()
    for k in (1, 7, 12):
        tabs2[k] = S.u01(L * L, 210 + k).reshape(L, L); sc2[k] = 2.0 + k
        if kind == "diff":
            lp.set_factor_cost(p[k], td, L, L, sc2[k])
        else:
            lp.set_factor_cost(p[k], L, L, tabs2[k])
    if kind == "diff":
        lp.set_diff_table(td, D1)
    assert not lp._dirty
    lp.upload_costs(warm=True)
    assert lp._engine.schedules_built() == built and lp._engine.plan.h == handle
    assert np.array_equal(lp.duals(), duals)
    new, _, _, _ = _lp_grid(kind, D1, tabs2, un, sc2)
    new.set_reparametrization("anisotropic")
    new._duals_host = duals                                                   # started from the same duals (flat_model lays them over the costs)
    for it in range(3):
        lp.ComputePass(it); new.ComputePass(it)
        assert lp.LowerBound() == new.LowerBound()
    assert np.array_equal(lp.duals(), new.duals())
    assert lp._engine.schedules_built() == built
