"""lpmp_path_moves on the device against the numpy statement of the rule (tests/path_moves_cases.py).

Procedure: upload, set the duals (passes, or random numbers: the rule reads any duals), upload a starting labelling, move;
``download_primal`` — the unary labels and both slots of every pairwise factor — must be ``np.array_equal`` to
``path_moves_reference`` on the downloaded duals after EVERY group of every round (one prepared set per group, moved in turn), and
again after the whole move through one set.  The shapes are the smallest at which the kernel takes another path: label counts at
the edges of the wave (64), of the workgroup's stride (256) and the limit (512); rectangular tables with the members on either
side; both back-pointer widths; every pairwise kind and storage; ties, +inf entries and unset neighbours."""
import dataclasses

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import lp as LPM
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

import decode_cases as DC
import path_moves_cases as C

pytestmark = pytest.mark.gpu

ANISO = M.REPAM_ANISOTROPIC
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -2, -4


def _engine(m, passes=0, random_duals=None, **kw):
    e = E.Engine(0)
    e.upload(m, **kw)
    e.set_reparametrization(ANISO)
    if passes:
        e.compute_pass(passes)
    if random_duals is not None:
        e.upload_duals(np.random.default_rng(random_duals).random(m.dual_data.shape[0]))
    return e


def _differ(got, want):
    bad = np.argwhere(got != want)
    return bad[:8].tolist(), got[bad[:8, 0]].tolist(), want[bad[:8, 0]].tolist()


def _check_moves(e, m, groups, start, rounds=1, what=""):
    """``m``: the model the device computes on (float tables rounded).  Returns the labels after the move."""
    duals = e.download_duals()
    assert not np.any(np.isnan(duals)), what
    trace = []
    want = C.path_moves_reference(m, duals, start, groups, rounds=rounds, trace=trace)
    e.upload_primal(start)
    sets = [e.path_set([g]) for g in groups]
    for i, t in enumerate(trace):
        sets[i % len(groups)].move(1)
        got = e.download_primal()
        assert np.array_equal(got, t), (what, "round %d group %d" % divmod(i, len(groups))) + _differ(got, t)
    for s in sets:
        s.close()
    e.upload_primal(start)
    ps = e.path_set(groups)
    assert ps.n_groups == len(groups) and ps.n_paths == sum(len(g) for g in groups) and ps.longest == max([len(p) for g in groups for p in g], default=0)
    ps.move(rounds)
    got = e.download_primal()
    assert np.array_equal(got, want), (what, "whole move") + _differ(got, want)
    ps.close()
    return got


# name -> (model and groups, upload keywords, passes before the move (0: random duals))
KINDS = {
    "dense13": (lambda: C.ladder((13, 13, 13, 13), "dense", seed=3), {}, 2),
    "dense13_random_duals": (lambda: C.ladder((13, 13, 13, 13), "dense", seed=3), {}, 0),
    "dense_f32": (lambda: C.ladder((13, 9, 13, 9), "dense_f32", seed=4), {"table_precision": "f32"}, 2),
    "dense_f32_round": (lambda: C.ladder((13, 9, 13, 9), "dense", seed=5), {"table_precision": "f32_round"}, 2),
    "potts13": (lambda: C.ladder((13, 13, 13, 13), "potts", seed=6), {}, 2),
    "shared13": (lambda: C.ladder((13, 7, 13, 7), "shared", seed=7), {}, 2),
    "diff_full": (lambda: C.ladder((40, 33, 40, 33), "diff", seed=8), {}, 2),
    "diff_banded": (lambda: C.ladder((40, 40, 40, 40), "diff_banded", seed=9), {}, 2),
    "diff_shift": (lambda: C.diff_shift_case(), {}, 2),
    "mixed": (lambda: C.mixed_path_case(), {}, 2),
    "rows_layout": (lambda: C.ladder((13, 13, 13, 13), "dense", seed=3), {"rows_layout": True}, 2),
    "sides_none": (lambda: C.ladder((5, 9, 7, 9, 5), "dense", seed=10, flip="none"), {}, 0),
    "sides_all": (lambda: C.ladder((5, 9, 7, 9, 5), "dense", seed=11, flip="all"), {}, 0),
    "sides_alternate": (lambda: C.ladder((5, 9, 7, 9, 5), "dense", seed=12, flip="alternate"), {}, 0),
    "length1": (lambda: C.ladder((5,), "dense", seed=13), {}, 0),
    "length2": (lambda: C.ladder((5, 6), "dense", seed=14), {}, 0),
    "length3": (lambda: C.ladder((5, 6, 4), "dense", seed=15), {}, 0),
    "length300": (lambda: C.long_case(), {}, 2),
    "rect_both_forms": (lambda: C.rect_case(), {}, 0),
    "pair512": (lambda: C.pair512_case(), {}, 0),
    "ties_dense": (lambda: C.ladder((6, 6, 6, 6), "dense", seed=16, ints=True), {}, 0),
    "ties_potts": (lambda: C.ladder((6, 6, 6, 6), "potts", seed=17, ints=True), {}, 0),
    "ties_diff": (lambda: C.ladder((6, 6, 6, 6), "diff", seed=18, ints=True), {}, 0),
    "inf_tables": (lambda: C.inf_case(), {}, 0),
    "all_inf": (lambda: C.all_inf_case(), {}, 0),
}


@pytest.mark.parametrize("name", sorted(KINDS))
def test_moves_match_the_statement(name):
    make, kw, passes = KINDS[name]
    m, groups = make()
    if name.startswith("ties") or name == "all_inf":      # the duals are the costs themselves (zero messages): quantised, ties everywhere
        e = _engine(m, **kw)
    else:
        e = _engine(m, passes, None if passes else 1000 + len(name), **kw)
    if "rows_layout" in kw:
        assert e.rows_layout
    ref = m
    if "table_precision" in kw:
        assert e.table_precision() == kw["table_precision"]
        ref = m.with_f32_tables()
    got = _check_moves(e, ref, groups, C.random_primal(m, 7), rounds=2, what=name)
    if name == "all_inf":
        assert got[2, 0] == 0
    if name == "rect_both_forms":   # the wave form and the workgroup form in one group, one- and two-byte back-pointers in one path
        ps = e.path_set(groups)
        assert ps.scratch_bytes == (40 + 9 + 70) + (300 + 7 * 2 + (257 + 1)) and ps.longest == 4     # (the two-byte run starts at an even byte)
        ps.close()
    e.close()


@pytest.mark.parametrize("L", [1, 2, 3, 8, 31, 32, 33, 64, 65, 130, 256, 257, 512])
def test_label_counts(L):
    """three members of L labels on alternating sides, an off-path neighbour each; random duals (passes on more than 256 labels are
    beyond the sweep kernels).  512 labels: DIFF factors (a dense table would be 2 MB each)"""
    m, groups = C.labels_case(L, "dense" if L < 512 else "diff")
    e = _engine(m, 0, L)
    _check_moves(e, m, groups, C.random_primal(m, L), rounds=1, what="L=%d" % L)
    ps = e.path_set(groups)
    assert ps.scratch_bytes == 2 * L * (1 if L <= 256 else 2)
    ps.close()
    e.close()


@pytest.mark.parametrize("order", ["row_major", "colour_major"])
@pytest.mark.parametrize("shape,rounds", [((7, 6), 3), ((12, 9), 2), ((12, 9), 1)])
def test_grids(shape, rounds, order):
    H, W = shape
    m = C.grid(H, W, 5, order)
    e = _engine(m, 3)
    e.decode_primal(0, 0)
    start = e.download_primal()
    groups = S.grid_paths(H, W, order)
    got = _check_moves(e, m, groups, start, rounds=rounds, what=(shape, order))
    # state: evaluate_primal prices the device's labels; a read-out agrees; the energy did not rise and stays above the bound
    assert e.check_primal_consistency()
    cost, want, before = e.evaluate_primal(), C.energy(m, got), C.energy(m, start)
    assert abs(cost - want) <= 1e-9 * max(1.0, abs(want))
    assert want <= before + 1e-9 * max(1.0, abs(before)) and cost >= e.lower_bound() - 1e-9 * max(1.0, abs(cost))
    r = e.readout()
    assert np.array_equal(r.labels(), got[:H * W, 0])
    r.close()
    e.close()


def test_star_paths_through_the_hub():
    m = DC.star()
    e = _engine(m, 2)
    groups = [[[0, 35, 1]], [[70, 35, 2]], [[3], [4], [5, ]], [[35]], [[36, 35, 34]]]
    _check_moves(e, m, groups, C.random_primal(m, 1), rounds=2, what="star")
    e.close()


def test_unlisted_parts_and_a_labeling_list_factor_elsewhere():
    # only two rows and a column of a grid are listed
    m = C.grid(7, 6, 5, "colour_major")
    var = S.grid_variable_order(7, 6, "colour_major")
    e = _engine(m, 2)
    _check_moves(e, m, [[var[1].tolist(), var[4, 1:5].tolist()], [var[2:6, 3].tolist()]], C.random_primal(m, 2), rounds=2, what="partial")
    e.close()
    # the Potts grid of c5_model with labeling-list factors beside it: the rounding code refuses the model, so the labels live in
    # the array of unset labels and are read through a read-out; the grid is the Potts grid_model of the same seed, factor for factor
    H, W, L = 5, 4, 4
    m5 = S.c5_model(H, W, L, 12, 6, 3, seed=2, window=12)
    mg = S.grid_model(H, W, L, pairwise="potts", order="colour_major", seed=2)
    n = mg.n_factors
    assert np.array_equal(m5.f_kind[:n], mg.f_kind) and np.array_equal(m5.const_data[:mg.const_data.shape[0]], mg.const_data)
    assert np.array_equal(m5.dual_data[:mg.dual_data.shape[0]], mg.dual_data)
    e = _engine(m5, 2)
    with pytest.raises(E.EngineError):
        e.download_primal()
    groups = S.grid_paths(H, W, "colour_major")
    duals = e.download_duals()[:mg.dual_data.shape[0]]
    unset = np.stack([mg.f_dim0, np.where(mg.f_kind == M.F_VECTOR, 0, mg.f_dim1)], 1).astype(np.int32)
    trace = []
    C.path_moves_reference(mg, duals, unset, groups, rounds=2, trace=trace)
    ps = e.path_set(groups)
    r = e.readout(np.arange(H * W))
    ps.move(2)
    assert np.array_equal(r.labels(), trace[-1][:H * W, 0])
    ps.close(); r.close()
    e.close()


def test_an_unset_neighbour_is_clamped():
    """rail B of the ladder holds no label (the dimension, as after an upload): its members count with their LAST label"""
    m, groups = C.ladder((5, 9, 7), "dense", seed=21)
    e = _engine(m, 0, 5)
    unset = e.download_primal()
    assert np.array_equal(unset[:6, 0], m.f_dim0[:6])
    got = _check_moves(e, m, groups[:1], unset, rounds=1, what="unset")
    assert np.all(got[:3, 0] < m.f_dim0[:3]) and np.array_equal(got[3:6], unset[3:6])
    # a negative stray label counts as label 0
    stray = unset.copy()
    stray[3:6, 0] = -7
    _check_moves(e, m, groups[:1], stray, rounds=1, what="stray")
    e.close()


def test_a_move_writes_labels_only():
    for make, kw in ((lambda: (C.grid(9, 7, 8, "colour_major"), S.grid_paths(9, 7, "colour_major")), {}),
                     (lambda: C.ladder((13, 13, 13, 13), "dense", seed=3), {"rows_layout": True}), (lambda: C.mixed_path_case(), {})):
        m, groups = make()
        e = _engine(m, 3, **kw)
        e.enable_kernel_timing(True)
        e.compute_pass(1)
        e.upload_primal(C.random_primal(m, 3))
        built = e.schedules_built()
        ps = e.path_set(groups)
        assert e.schedules_built() == built + 1                # the create is counted once
        lb0 = e.lower_bound()
        d0, f0, kt0 = e.download_duals(), e.factor_lower_bounds(), e.kernel_timing()
        lb0b, rec0b = e.lower_bound(), e.lower_bound_recomputed()
        ps.move(1); ps.move(3)
        assert e.schedules_built() == built + 1                # a move plans nothing
        lb1, rec1 = e.lower_bound(), e.lower_bound_recomputed()
        d1, f1, kt1 = e.download_duals(), e.factor_lower_bounds(), e.kernel_timing()
        assert d0.tobytes() == d1.tobytes() and f0.tobytes() == f1.tobytes() and kt0 == kt1
        assert np.float64(lb0).tobytes() == np.float64(lb0b).tobytes() == np.float64(lb1).tobytes()
        assert rec1 <= rec0b                                   # the moves made no tracked bound stale
        # and a pass afterwards continues from the same duals as on an engine that never moved
        f = _engine(m, 3, **kw)
        f.compute_pass(1)
        e.compute_pass(1); f.compute_pass(1)
        assert np.array_equal(e.download_duals(), f.download_duals())
        ps.close()
        e.close(); f.close()


def test_a_move_runs_on_the_costs_of_the_moment():
    import recost_cases as RC
    A = RC.grid(9, 7, 8)
    B = RC.recost(A, 77)
    groups = S.grid_paths(9, 7, "colour_major")
    e = _engine(A, 2)
    ps = e.path_set(groups)
    built = e.schedules_built()

    def check(m, what):
        start = C.random_primal(m, 4)
        e.upload_primal(start)
        ps.move(2)
        got, want = e.download_primal(), C.path_moves_reference(m, e.download_duals(), start, groups, rounds=2)
        assert np.array_equal(got, want), (what,) + _differ(got, want)

    check(A, "A")
    e.upload_costs(const=B.const_data)                         # warm: the messages stay
    check(dataclasses.replace(A, const_data=B.const_data, _keep=[]), "warm")
    e.upload_costs(const=B.const_data, duals=B.dual_data)      # cold
    e.compute_pass(2)
    check(B, "cold")
    p = int(np.flatnonzero(B.f_kind != M.F_VECTOR)[3])
    coff = B.const_offsets()
    T = np.random.default_rng(5).random(coff[p + 1] - coff[p])
    e.set_constants([p], T[None])
    c2 = B.const_data.copy()
    c2[coff[p]:coff[p + 1]] = T
    check(dataclasses.replace(B, const_data=c2, _keep=[]), "set_constants")
    assert e.schedules_built() == built
    ps.close(); e.close()
    # pool values
    m, groups = C.ladder((13, 7, 13, 7), "shared", seed=7)
    e = _engine(m, 2)
    ps = e.path_set(groups)
    m2 = m.with_pool(m.sh_data * 0.5 + 0.25)
    e.upload_shared_pool(m2.sh_data)
    start = C.random_primal(m2, 6)
    e.upload_primal(start)
    ps.move(1)
    assert np.array_equal(e.download_primal(), C.path_moves_reference(m2, e.download_duals(), start, groups))
    ps.close(); e.close()
    # moved windows: the shifts and the duals of the moment
    m, groups = C.diff_shift_case()
    e = _engine(m, 2)
    ps = e.path_set(groups)
    ws = e.window_set()
    delta = np.random.default_rng(8).integers(-3, 4, ws.n)
    m2, d2 = M.move_windows(m, e.download_duals(), None, delta)
    ws.move(delta)
    assert np.array_equal(e.download_duals(), d2)
    start = C.random_primal(m2, 9)
    e.upload_primal(start)
    ps.move(2)
    assert np.array_equal(e.download_primal(), C.path_moves_reference(m2, d2, start, groups, rounds=2))
    ws.close(); ps.close(); e.close()


def test_a_move_settles_passes_that_ran_ahead(monkeypatch):
    """as tests/test_decode_gpu.py: with speculation on the device is passes ahead of the caller; the move first settles"""
    monkeypatch.setenv("LPMP_ROT_BANDS", "6")
    H, W = 40, 36
    m = S.grid_model(H, W, 32, order="colour_major", seed=6)
    groups = S.grid_paths(H, W, "colour_major")[:1]
    e, f = E.Engine(0), E.Engine(0)
    for x in (e, f):
        x.upload(m); x.set_reparametrization(ANISO)
        x.lower_bound()
    e.set_speculation(8)
    for k in range(4):
        e.compute_pass(1); f.compute_pass(1)
    st = e.speculation_stats()
    assert st["batches"] == 2 and st["passes_launched"] == 6 and st["rollbacks"] == 0, st
    pe, pf = e.path_set(groups), f.path_set(groups)
    start = C.random_primal(m, 11)
    pe.move(1)                                                  # settles; the labels are still unset here
    assert e.speculation_stats()["rollbacks"] == 1
    assert np.array_equal(e.download_duals(), f.download_duals())
    for x, ps in ((e, pe), (f, pf)):
        x.upload_primal(start); ps.move(1)
    got = e.download_primal()
    assert np.array_equal(got, f.download_primal())
    assert np.array_equal(got, C.path_moves_reference(m, e.download_duals(), start, groups))
    pe.close(); pf.close(); e.close(); f.close()


def test_error_returns_stale_and_empty_sets_and_the_lp_mirror():
    m, groups = C.ladder((5, 6, 4), "dense", seed=15)
    e = E.Engine(0)
    with pytest.raises(E.EngineError) as ei:
        e.path_set(groups)
    assert ei.value.code == ERR_STATE
    e.upload(m)
    ps = e.path_set(groups)
    with pytest.raises(E.EngineError) as ei:
        ps.move(-1)
    assert ei.value.code == ERR_INVALID
    with pytest.raises(E.EngineError) as ei:
        e.path_set([[[0, 2]]])
    assert ei.value.code == ERR_INVALID and "no pairwise factor joins" in str(ei.value)
    start = C.random_primal(m, 1)
    e.upload_primal(start)
    ps.move(0)                                                  # rounds = 0: nothing moves
    assert np.array_equal(e.download_primal(), start)
    for empty in ([], [[], []]):
        es = e.path_set(empty)
        assert (es.n_groups, es.n_paths, es.longest, es.scratch_bytes) == (len(empty), 0, 0, 0)
        es.move(3)
        assert np.array_equal(e.download_primal(), start)
        es.close()
    ps.move(1)                                                  # no weights needed: a move reads duals, constants and labels
    assert np.array_equal(e.download_primal(), C.path_moves_reference(m, m.dual_data, start, groups))
    # a stale set
    e.upload(m)
    with pytest.raises(E.EngineError) as ei:
        ps.move(1)
    assert ei.value.code == ERR_STATE
    ps.close(); ps.close()
    mc = S.multicut_triangle_model(6, 4, seed=1)
    e.upload(mc)
    with pytest.raises(E.EngineError) as ei:
        e.path_set([[[0]]])
    assert ei.value.code == ERR_UNSUPPORTED and "factor 0 " in str(ei.value)
    e.close()
    # LP mirror: the README quick-start model (optimum 1.0 at labels (0, 0) or (1, 1)); a path over both variables finds it from (0, 1)
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.PairwiseSimplexFactor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    lp = LPM.LP(LPM.FMC("SRMP", [U, P], [ML, MR]))
    u1, u2 = lp.add_factor(U, [0.0, 1.0]), lp.add_factor(U, [1.0, 0.0])
    p = lp.add_factor(P, 2, 2, [[0.0, 1.0], [1.0, 0.0]])
    lp.add_message(ML, u1, p); lp.add_message(MR, u2, p)
    lp.AddFactorRelation(u1, p); lp.AddFactorRelation(p, u2)
    lp.set_reparametrization("anisotropic")
    lp.ComputePass(0)
    lp.decode_primal(0, 0)
    cost = lp.path_moves([[[u1, u2]]], rounds=1)
    pr = lp.primal()
    assert cost == 1.0 and lp.CheckPrimalConsistency() and list(pr[p]) == [pr[u1, 0], pr[u2, 0]] == [0, 0]


# ---- far offsets: the live model behind 2^31 elements of padding (tests/far_offset_cases.py) ------------------------------------
def test_paths_behind_far_offsets():
    """a DIFF_SHIFT ladder and a dense one behind 32 768 isolated 1 x 65 536 dense factors: every dual and constant offset of the
    path records lies past 2^31 elements.  Labels against the statement on the small model"""
    import torch
    import far_offset_cases as F
    need, free = F.FarBuffers.bytes_needed("P31"), torch.cuda.mem_get_info()[0]
    assert free >= need + F.GIB, "the device reports %.1f GiB free, the padding needs %.1f GiB" % (free / F.GIB, need / F.GIB)
    bufs = F.FarBuffers("P31")
    try:
        for make in (C.diff_shift_case, lambda: C.ladder((13, 9, 70, 9), "dense", seed=31)):
            m, groups = make()
            far = F.pad_front(m, bufs.n_pad)
            n_pad = bufs.n_pad
            assert int(far.const_offsets()[n_pad]) >= 2**31 and int(far.dual_offsets()[n_pad]) >= 2**31
            duals = np.random.default_rng(3).random(m.dual_data.shape[0])
            cp, dp = bufs.load(m, dual=duals)
            e = E.Engine(0)
            e.upload(far, const_dev=cp, dual_dev=dp, keep=(bufs.const, bufs.dual))
            start = C.random_primal(m, 5)
            pr = e.download_primal()
            pr[n_pad:] = start
            e.upload_primal(pr)
            ps = e.path_set([[[u + n_pad for u in p] for p in g] for g in groups])
            ps.move(2)
            got = e.download_primal()
            want = C.path_moves_reference(m, duals, start, groups, rounds=2)
            assert np.array_equal(got[n_pad:], want), _differ(got[n_pad:], want)
            assert np.array_equal(got[:n_pad], pr[:n_pad])
            e.synchronize()
            assert np.array_equal(bufs.dual_tail(), duals) and bufs.dual_padding_nonzero() == 0
            ps.close(); e.close()
            bufs.reset()
    finally:
        bufs.const = bufs.dual = None
        torch.cuda.empty_cache()
