"""lpmp_readout_* on the device: labels and unaries against ``download_primal`` / the packed duals, beliefs against the
numpy statement of the rule (tests/readout_cases.py) on the engine's own downloaded duals.

Every comparison is ``np.array_equal``; what a call must leave untouched (the padding of a row, a sentinel row behind the last one)
is compared by the bits of a NaN sentinel.  The shapes are the smallest at which the kernels take another path: label counts at the
edges of the lane groups (4 / 8 / 16 / 32 lanes), of the 64-lane stride and beyond the 256 labels a wave holds in registers;
rectangular tables with the unary on either side, also with more peer labels than the group has lanes; every pairwise kind and
storage; 0, 1, 4 and 9 links."""
import numpy as np
import pytest
import torch

from lp_mp_amd import engine as E
from lp_mp_amd import lp as LPM
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import decode_cases as DC
import readout_cases as R

pytestmark = pytest.mark.gpu

ANISO, UNIFORM = M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -2, -4
SENTINEL = np.array([0x7FF8DEAD0000BEEF], np.uint64).view(np.float64)[0]      # a NaN with a payload
SENTINEL_I32 = np.int32(-0x5EADBEF)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _engine(m, passes=2, mode=ANISO, **kw):
    e = E.Engine(0)
    e.upload(m, **kw)
    e.set_reparametrization(mode)
    if passes:
        e.compute_pass(passes)
    return e


def _device_rows(call, n, stride):
    """``call(dst_dev, stride)`` into a torch tensor of n + 1 rows filled with the sentinel; returns the array afterwards"""
    t = torch.from_numpy(np.full((n + 1) * stride, SENTINEL)).cuda()
    torch.cuda.synchronize()
    assert call(t.data_ptr(), stride) is None
    return t.cpu().numpy().reshape(n + 1, stride)          # (.cpu() waits for the null stream only: callers synchronise the engine first)


def _check_rows(got_dev, want, what):
    """a device destination [n + 1, stride] against ``want`` [n, stride] (NaN = not written): written entries equal, everything
    else — padding and the row behind the last — still the sentinel, bit for bit"""
    n = want.shape[0]
    written = ~np.isnan(want)
    assert np.array_equal(got_dev[:n][written], want[written]), what
    assert np.all(_bits(got_dev[:n][~written]) == _bits(SENTINEL)), what
    assert np.all(_bits(got_dev[n]) == _bits(SENTINEL)), what


def _check_beliefs(e, m, what, factors=None):
    """host and device destination of ``beliefs`` against the statement on the engine's own duals; returns the host array"""
    duals = e.download_duals()
    assert not np.any(np.isnan(duals)), what
    want = R.beliefs_np(m, duals, factors)
    r = e.readout(factors)
    got = r.beliefs()
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert np.array_equal(got, want, equal_nan=True), (what, bad[:6].tolist())
    stride = r.max_labels + 3
    dev = _device_rows(lambda p, s: (r.beliefs(p, s), e.synchronize())[0], r.n, stride)
    _check_rows(dev, R.beliefs_np(m, duals, factors, stride=stride), what)
    r.close()
    return got


# ---- labels / vectors ------------------------------------------------------------------------------------------------------------
LV_MODELS = {"grid5x6x3": lambda: R.grid(5, 6, 3), "ragged": lambda: R.ragged()}


def _check_labels_vectors(e, m, lists, what):
    duals = e.download_duals()
    primal = e.download_primal()
    for factors in lists:
        r = e.readout(factors)
        fs = R.unaries(m) if factors is None else list(factors)
        assert r.n == len(fs) and r.max_labels == max(int(m.f_dim0[f]) for f in fs)
        want_l = primal[fs, 0]
        want_v = R.vectors_np(m, duals, fs)
        # host destinations
        assert np.array_equal(r.labels(), want_l), what
        assert np.array_equal(r.vectors(), want_v, equal_nan=True), what
        # device destinations: stride Lmax + 3 and a sentinel row behind the last
        stride = r.max_labels + 3
        dev = _device_rows(lambda p, s: (r.vectors(p, s), e.synchronize())[0], r.n, stride)
        _check_rows(dev, R.vectors_np(m, duals, fs, stride=stride), what)
        t = torch.from_numpy(np.full(r.n + 1, SENTINEL_I32, np.int32)).cuda()
        torch.cuda.synchronize()
        assert r.labels(t.data_ptr()) is None
        e.synchronize()
        got = t.cpu().numpy()
        assert np.array_equal(got[:r.n], want_l) and got[r.n] == SENTINEL_I32, what
        r.close()
    return primal


@pytest.mark.parametrize("name", sorted(LV_MODELS))
def test_labels_and_vectors(name):
    m = LV_MODELS[name]()
    us = R.unaries(m)
    perm = np.random.default_rng(3).permutation(us)[: max(3, len(us) * 2 // 3)].tolist()
    perm.insert(2, perm[0])                                   # one factor listed twice
    lists = (perm, None)
    e = _engine(m)
    pr = _check_labels_vectors(e, m, lists, "before any decode")
    assert np.array_equal(pr[us, 0], m.f_dim0[us])            # all unset: the dimension
    e.decode_primal(0, 1)
    pr = _check_labels_vectors(e, m, lists, "after decode_primal")
    assert np.all(pr[us, 0] < m.f_dim0[us])
    e.close()
    mp = S.grid_model(5, 6, 3, compute_primal=True) if name == "grid5x6x3" else None
    if mp is not None:
        e = _engine(mp)
        e.compute_pass_and_primal(1)
        pr = _check_labels_vectors(e, mp, lists, "after compute_pass_and_primal")
        assert np.all(pr[us, 0] < mp.f_dim0[us])
        e.close()


# ---- beliefs ---------------------------------------------------------------------------------------------------------------------
# name -> (model the engine gets, upload keywords, model of the statement or None: the same)
BELIEF_CASES = {}
for _L in (2, 7, 32, 33, 65, 300):
    for _kind in ("dense", "potts", "shared", "diff"):
        BELIEF_CASES["%s%d" % (_kind, _L)] = (lambda L=_L, kind=_kind: DC.labels_case(L, kind), {}, None)
BELIEF_CASES.update({
    "dense_f32": (lambda: DC.f32_case(), {"table_precision": "f32"}, None),
    "dense_f32_65": (lambda: DC.labels_case(65).with_f32_tables(), {"table_precision": "f32"}, None),
    "dense_f32_round": (lambda: DC.labels_case(33), {"table_precision": "f32_round"}, lambda: DC.labels_case(33).with_f32_tables()),
    "diff_banded": (lambda: DC.diff_case(True), {}, None),
    "diff_full": (lambda: DC.diff_case(False), {}, None),
    "mixed": (lambda: DC.mixed_case(), {}, None),                      # dense + shared + Potts + DIFF peers of one unary; an isolated unary
    "rect4x7": (lambda: R.rect_chain(), {}, None),
    "rect5x9": (lambda: DC.rect_case(5, 9), {}, None),
    "rect40x33": (lambda: DC.rect_case(40, 33), {}, None),
    "rect5x70": (lambda: DC.rect_case(5, 70), {}, None),               # more peer labels than the group has lanes
    "rect70x300": (lambda: DC.rect_case(70, 300), {}, None),
    "hub9": (lambda: R.hub(), {}, None),
    "inf_entries": (lambda: DC.inf_tables_case(), {}, None),
    "rows_layout": (lambda: DC.labels_case(13), {"rows_layout": True}, None),
    "rows_layout_grid": (lambda: R.grid(9, 7, 8, order="colour_major"), {"rows_layout": True}, None),
    "grid_colour_major": (lambda: R.grid(9, 7, 8, order="colour_major"), {}, None),
    "ragged": (lambda: R.ragged(), {}, None),
})


@pytest.mark.parametrize("name", sorted(BELIEF_CASES))
def test_beliefs_match_the_statement(name):
    make, kw, ref = BELIEF_CASES[name]
    m = make()
    e = _engine(m, **kw)
    if "rows_layout" in kw:
        assert e.rows_layout
    if "table_precision" in kw:
        assert e.table_precision() == kw["table_precision"]
    _check_beliefs(e, ref() if ref else m, name)
    e.close()


@pytest.mark.parametrize("name", ["dense7", "potts33", "shared65", "diff32", "mixed", "hub9", "rect5x9"])
def test_beliefs_in_the_uniform_mode(name):
    make, kw, _ = BELIEF_CASES[name]
    m = make()
    e = _engine(m, mode=UNIFORM, **kw)
    _check_beliefs(e, m, name)
    e.close()


def test_link_counts_and_a_permuted_list():
    m = DC.mixed_case()
    lists = R.message_lists(m)
    us = R.unaries(m)
    assert sorted({len(lists[u]) for u in us} & {0, 1}) == [0, 1]
    small = R.message_lists(DC.labels_case(7))                # (the graph of every ``<kind><L>`` case above)
    assert {len(small[u]) for u in R.unaries(DC.labels_case(7))} >= {1, 4} and len(R.message_lists(R.hub())[4]) == 9
    e = _engine(m)
    perm = [3, 8, 0, 3, 9, 5]                                  # unary 3 twice; 8 and 9 are isolated (9: all +inf)
    got = _check_beliefs(e, m, "mixed, permuted", perm)
    assert np.array_equal(got[0], got[3], equal_nan=True)
    th = R.vectors_np(m, e.download_duals(), [8], stride=got.shape[1])
    assert np.array_equal(got[1], th[0], equal_nan=True)       # a unary without messages gets theta
    assert np.all(np.isinf(got[4, :3]))
    e.close()


def test_all_inf_row():
    """a table with +inf entries and one all-+inf row.  The duals are those of two passes on the model with that row finite (with the
    row +inf a pass makes NaN duals: readout_cases.inf_row_pair); the row is then set on the device"""
    a, b = R.inf_row_pair()
    p = R.inf_row_factor(a)
    e = _engine(a)
    L = int(a.f_dim0[p])
    coff = b.const_offsets()
    e.set_constants([p], b.const_data[coff[p]:coff[p + 1]][None])
    got = _check_beliefs(e, b, "all-+inf row")
    u = int(a.m_left[[k for k in range(a.n_messages) if int(a.m_right[k]) == p and a.mtypes[int(a.m_type[k])].param == 0][0]])
    row = R.unaries(a).index(u)
    assert np.isposinf(got[row, 2]) and np.isfinite(np.delete(got[row, :L], 2)).all()
    e.close()


def test_nothing_moves():
    for make, kw in ((lambda: R.grid(9, 7, 8, order="colour_major"), {}), (lambda: DC.labels_case(13), {"rows_layout": True}), (lambda: DC.mixed_case(), {})):
        m = make()
        e = _engine(m, **kw)
        e.decode_primal(0, 0)
        lb0, rec0 = e.lower_bound(), e.lower_bound_recomputed()
        d0, p0 = e.download_duals(), e.download_primal()
        lb0b, rec0b = e.lower_bound(), e.lower_bound_recomputed()
        r = e.readout()
        built0 = e.schedules_built()
        r.labels(); r.vectors()
        assert e.schedules_built() == built0                   # nothing is built at create or by labels / vectors
        r.beliefs()
        built1 = e.schedules_built()
        assert built1 == built0 + 1                            # the link tables, once
        r.beliefs(); r.labels(); r.vectors()
        assert e.schedules_built() == built1
        lb1, rec1 = e.lower_bound(), e.lower_bound_recomputed()
        assert d0.tobytes() == e.download_duals().tobytes() and np.array_equal(p0, e.download_primal())
        assert np.float64(lb0).tobytes() == np.float64(lb0b).tobytes() == np.float64(lb1).tobytes()
        print("bounds recomputed: after the passes", rec0, "again", rec0b, "after the read-outs", rec1)
        assert rec0b == 0                                      # every bound is tracked: a read-out that made one stale would show
        assert rec1 == rec0b
        # and a pass afterwards continues from the same duals as on an engine that never read anything out
        f = _engine(m, **kw)
        e.compute_pass(1); f.compute_pass(1)
        assert np.array_equal(e.download_duals(), f.download_duals())
        r.close(); e.close(); f.close()


def test_beliefs_settle_passes_that_ran_ahead(monkeypatch):
    monkeypatch.setenv("LPMP_ROT_BANDS", "6")          # the joined chain on a small model (as tests/test_speculation_gpu.py does)
    m = S.grid_model(40, 36, 32, order="colour_major", seed=6)
    e = E.Engine(0)
    e.upload(m); e.set_reparametrization(ANISO)
    e.lower_bound()
    e.set_speculation(4)
    r = e.readout()
    e.compute_pass(1); e.compute_pass(1)
    print("speculation:", e.speculation_stats())
    got = r.beliefs()
    o = Oracle(m)
    o.set_reparametrization(ANISO)
    o.ComputePass(2)
    assert np.array_equal(got, R.beliefs_np(m, o.duals()), equal_nan=True)
    assert np.array_equal(e.download_duals(), o.duals())
    r.close(); e.close()
    # the caller stopped INSIDE a batch: the first single pass launched two, the read-out rolls back to the one asked for
    f = E.Engine(0)
    f.upload(m); f.set_reparametrization(ANISO)
    f.lower_bound()
    f.set_speculation(4)
    r = f.readout()
    f.compute_pass(1)
    st = f.speculation_stats()
    assert st["passes_launched"] == 2 and st["rollbacks"] == 0, st
    got = r.beliefs()
    assert f.speculation_stats()["rollbacks"] == 1
    o = Oracle(m)
    o.set_reparametrization(ANISO)
    o.ComputePass(1)
    assert np.array_equal(got, R.beliefs_np(m, o.duals()), equal_nan=True)
    r.close(); f.close()


def test_lifetime_across_new_costs_and_models():
    import recost_cases as RC
    A = RC.grid(9, 7, 8)
    B = RC.recost(A, 77)
    e = _engine(A)
    r = e.readout()
    sub = e.readout([5, 1, 5])
    assert np.array_equal(r.beliefs(), R.beliefs_np(A, e.download_duals()), equal_nan=True)
    built = e.schedules_built()
    e.upload_costs(const=B.const_data, duals=B.dual_data)      # cold
    assert np.array_equal(r.vectors(), R.vectors_np(B, B.dual_data, R.unaries(B)), equal_nan=True)
    assert np.array_equal(r.labels(), B.f_dim0[R.unaries(B)])  # labels are unset after new costs
    e.compute_pass(2)
    assert np.array_equal(r.beliefs(), R.beliefs_np(B, e.download_duals()), equal_nan=True)
    new = np.random.default_rng(5).random((2, 8))
    e.set_vectors([1, 5], new)
    d = e.download_duals()
    assert np.array_equal(sub.vectors(), new[[1, 0, 1]])
    assert np.array_equal(r.beliefs(), R.beliefs_np(B, d), equal_nan=True)
    assert np.array_equal(sub.beliefs(), R.beliefs_np(B, d, [5, 1, 5]), equal_nan=True)
    assert e.schedules_built() == built + 1                    # (the link tables of `sub`)
    # pool values
    m = DC.labels_case(13, "shared")
    e2 = _engine(m)
    r2 = e2.readout()
    assert np.array_equal(r2.beliefs(), R.beliefs_np(m, e2.download_duals()), equal_nan=True)
    m2 = m.with_pool(m.sh_data * 0.5 + 0.25)
    e2.upload_shared_pool(m2.sh_data)
    assert np.array_equal(r2.beliefs(), R.beliefs_np(m2, e2.download_duals()), equal_nan=True)
    # a second upload ends the read-out; close still works
    e2.upload(m)
    for call in (r2.labels, r2.vectors, r2.beliefs):
        with pytest.raises(E.EngineError) as ei:
            call()
        assert ei.value.code == ERR_STATE
    r2.close()
    r3 = e2.readout()
    assert np.array_equal(r3.vectors(), R.vectors_np(m, m.dual_data, R.unaries(m)), equal_nan=True)
    r3.close(); r.close(); sub.close(); e.close(); e2.close()


def test_device_destination_is_ordered_on_the_engines_stream():
    m = R.grid(9, 7, 8, order="colour_major")
    s = torch.cuda.Stream()
    e = E.Engine(0)
    e.set_stream(s.cuda_stream)
    e.upload(m); e.set_reparametrization(ANISO)
    r = e.readout()
    stride = r.max_labels
    with torch.cuda.stream(s):
        t = torch.full((r.n, stride), float("nan"), dtype=torch.float64, device="cuda")
        lab = torch.full((r.n,), -1, dtype=torch.int32, device="cuda")
    e.compute_pass(2)
    e.decode_primal(0, 0)
    r.beliefs(t.data_ptr(), stride)
    r.labels(lab.data_ptr())
    s.synchronize()                                            # no Engine.synchronize()
    with torch.cuda.stream(s):
        got, got_l = t.cpu().numpy(), lab.cpu().numpy()
    assert np.array_equal(got, R.beliefs_np(m, e.download_duals()), equal_nan=True)
    assert np.array_equal(got_l, e.download_primal()[R.unaries(m), 0])
    r.close(); e.close()


def test_device_destination_does_not_wait_for_the_stream(monkeypatch):
    """pass, decode, read-outs into device arrays: the calls return while the pass is still running.  The pass is a joined chain
    launch (the path of every ordinary compute_pass on a 2-colour grid), N passes long; T is what it takes from call to completion.
    With the same work queued again the three read-out calls together must take less host time than T / 4: they are three kernel
    launches (tens of microseconds) against T of tens of milliseconds, while a call that waited for the stream would take about T."""
    import time
    monkeypatch.setenv("LPMP_ROT_BANDS", "6")          # the joined chain on a small model (as tests/test_speculation_gpu.py does)
    m = S.grid_model(40, 36, 32, order="colour_major", seed=6)
    e = E.Engine(0)
    e.upload(m); e.set_reparametrization(ANISO)
    assert e.plan.pass_rotates(ANISO)
    r = e.readout()
    L = r.max_labels
    lab = torch.empty(r.n, dtype=torch.int32, device="cuda")
    rows = torch.empty(r.n * L, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    N = 1000

    def readouts():
        r.labels(lab.data_ptr()); r.vectors(rows.data_ptr(), L); r.beliefs(rows.data_ptr(), L)

    e.compute_pass(N); e.decode_primal(0, 0); readouts(); e.synchronize()        # everything that is built on first use exists now
    t0 = time.perf_counter()
    e.compute_pass(N); e.synchronize()
    T = time.perf_counter() - t0
    t0 = time.perf_counter()
    e.compute_pass(N); e.decode_primal(0, 0)
    t1 = time.perf_counter()
    readouts()
    t2 = time.perf_counter()
    e.synchronize()
    t3 = time.perf_counter()
    print("N passes %.2f ms; queued in %.3f ms, read-out calls %.3f ms, drained after %.2f ms" % (T * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
    assert T > 0.01                                    # the queued work is long against a launch
    assert t1 - t0 < T / 4                             # (the pass and the decode themselves return without waiting)
    assert t2 - t1 < T / 4
    assert np.array_equal(lab.cpu().numpy(), e.download_primal()[R.unaries(m), 0])
    assert np.array_equal(rows.cpu().numpy().reshape(r.n, L), R.beliefs_np(m, e.download_duals()), equal_nan=True)
    r.close(); e.close()


def test_refusals():
    e = E.Engine(0)
    with pytest.raises(E.EngineError) as ei:
        e.readout()
    assert ei.value.code == ERR_STATE
    m = R.ragged()
    e.upload(m)
    for bad, word in (([0, m.n_factors], "out of range"), ([0, -1], "out of range"), ([1, int(np.flatnonzero(m.f_kind != M.F_VECTOR)[0])], "not a VECTOR")):
        with pytest.raises(E.EngineError) as ei:
            e.readout(bad)
        assert ei.value.code == ERR_INVALID and word in str(ei.value) and str(bad[1]) in str(ei.value)
    r = e.readout([2, 0])
    assert (r.n, r.max_labels) == (2, 33)
    for call in (r.vectors, r.beliefs):
        with pytest.raises(E.EngineError) as ei:
            call(stride=32)
        assert ei.value.code == ERR_INVALID and "32" in str(ei.value)
    assert r.vectors(stride=33).shape == (2, 33)
    empty = e.readout([])
    assert empty.n == 0 and empty.max_labels == 0
    assert empty.labels().shape == (0,) and empty.vectors().shape == (0, 0) and empty.beliefs(stride=4).shape == (0, 4)
    r.close(); empty.close()
    # a labeling message on a listed vector factor: no beliefs, naming the lowest such factor; labels and vectors work
    mc = R.labeling_model()
    e.upload(mc)
    touched = sorted({int(f) for k in range(mc.n_messages) for f in (mc.m_left[k], mc.m_right[k])})
    listed = [touched[-1], touched[1], touched[2]]
    r = e.readout(listed)
    with pytest.raises(E.EngineError) as ei:
        r.beliefs()
    assert ei.value.code == ERR_UNSUPPORTED and ("factor %d " % touched[1]) in str(ei.value)
    assert np.array_equal(r.vectors(), R.vectors_np(mc, mc.dual_data, listed), equal_nan=True)
    assert np.array_equal(r.labels(), mc.f_dim0[listed])
    assert np.array_equal(r.labels(), mc.f_dim0[listed])      # (the unset array is made once and remembered)
    r.close(); e.close()


def test_the_lp_mirror():
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.PairwiseSimplexFactor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    lp = LPM.LP(LPM.FMC("SRMP", [U, P], [ML, MR]))
    u1, u2 = lp.add_factor(U, [0.0, 1.0]), lp.add_factor(U, [1.0, 0.25])
    p = lp.add_factor(P, 2, 2, [[0.0, 1.0], [1.0, 0.0]])
    lp.add_message(ML, u1, p); lp.add_message(MR, u2, p)
    lp.AddFactorRelation(u1, p); lp.AddFactorRelation(p, u2)
    lp.set_reparametrization("anisotropic")
    lp.ComputePass(0)
    r = lp.readout([u2, u1])
    e = lp._ready()
    duals = e.download_duals()
    assert np.array_equal(r.vectors(), R.vectors_np(e.model, duals, [u2, u1]))
    assert np.array_equal(r.beliefs(), R.beliefs_np(e.model, duals, [u2, u1]))
    lp.decode_primal(0, 0)
    assert np.array_equal(r.labels(), lp.primal()[[u2, u1], 0])
    r.close()
