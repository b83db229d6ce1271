"""lpmp_forest_moves on the device against the numpy statement of the rule (tests/forest_moves_cases.py).

Procedure, as in tests/test_path_moves_gpu.py: upload, set the duals (passes, or random numbers: the rule reads any duals), upload
a starting labelling, move; ``download_primal`` must be ``np.array_equal`` to ``forest_moves_reference`` on the downloaded duals
after EVERY group of every round (one prepared set per group, moved in turn), and again after the whole move through one set.  The
shapes are the smallest at which the kernels take another path: label counts at the edges of the wave (64), of the workgroup's
stride (256) and the limit (512); rectangular tree edges that put both forms at one height; both back-pointer widths; fan-in from
1 to 70 children; 300 height levels; every pairwise kind and storage; ties, +inf entries and unset neighbours."""
import dataclasses

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import lp as LPM
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

import decode_cases as DC
import forest_moves_cases as C
import path_moves_cases as PC

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


def _scratch(m, groups):
    """9 * sum of d_parent over the non-root nodes of the largest group (every member with at most 256 labels)"""
    return max([9 * sum(int(m.f_dim0[q]) for q in par if q != -1) for _, par in groups], default=0)


def _check_moves(e, m, groups, start, rounds=1, what="", scratch=True):
    """``m``: the model the device computes on (float tables rounded).  Returns the labels after the move."""
    duals = e.download_duals()
    assert not np.any(np.isnan(duals)), what
    trace = []
    want = C.forest_moves_reference(m, duals, start, groups, rounds=rounds, trace=trace)
    e.upload_primal(start)
    sets = [e.forest_set([g]) for g in groups]
    for i, t in enumerate(trace):
        sets[i % len(groups)].move(1)
        got = e.download_primal()
        assert np.array_equal(got, t), (what, "round %d group %d" % divmod(i, len(groups))) + _differ(got, t)
    for s in sets:
        s.close()
    e.upload_primal(start)
    fs = e.forest_set(groups)
    info = E.Plan(m).forest_info(groups)
    assert fs.n_groups == len(groups) and fs.n_trees == info["n_trees"] and fs.max_height == info["max_height"]
    if scratch and max([int(m.f_dim0[u]) for un, _ in groups for u in un], default=0) <= 256:
        assert fs.scratch_bytes == _scratch(m, groups), what
    fs.move(rounds)
    got = e.download_primal()
    assert np.array_equal(got, want), (what, "whole move") + _differ(got, want)
    fs.close()
    return got


def _inf_groups():
    # path_moves_cases.inf_case: edges 0-1 (all +inf into label 2 of variable 1), 2-1, 2-3, 0-4, 5-2, 4-5; rooted at 2, variable 4 apart
    return [(np.asarray([2, 1, 3, 5, 0], np.int32), np.asarray([-1, 2, 2, 2, 1], np.int32)), (np.asarray([4], np.int32), np.asarray([-1], np.int32))]


T7 = C.TREE7
# name -> (model and groups, upload keywords, passes before the move (0: random duals))
KINDS = {
    "dense13": (lambda: C.tree_model(T7, (13,) * 7, "dense", seed=3), {}, 2),
    "dense13_random_duals": (lambda: C.tree_model(T7, (13,) * 7, "dense", seed=3), {}, 0),
    "dense_f32": (lambda: C.tree_model(T7, (13, 9, 13, 9, 13, 9, 5), "dense_f32", seed=4), {"table_precision": "f32"}, 2),
    "dense_f32_round": (lambda: C.tree_model(T7, (13, 9, 13, 9, 13, 9, 5), "dense", seed=5), {"table_precision": "f32_round"}, 2),
    "rows_layout": (lambda: C.tree_model(T7, (13,) * 7, "dense", seed=3), {"rows_layout": True}, 2),
    "potts13": (lambda: C.tree_model(T7, (13,) * 7, "potts", seed=6), {}, 2),
    "shared13": (lambda: C.tree_model(T7, (13, 7, 13, 7, 13, 7, 13), "shared", seed=7), {}, 2),
    "diff_full": (lambda: C.tree_model(T7, (40, 33, 40, 33, 40, 33, 40), "diff", seed=8), {}, 2),
    "diff_banded": (lambda: C.tree_model(T7, (40,) * 7, "diff_banded", seed=9), {}, 2),
    "diff_shift": (lambda: C.diff_shift_tree(), {}, 2),
    "all_kinds": (lambda: C.tree_model(T7, (13,) * 7, ("dense", "potts", "shared", "diff", "diff_banded", "dense"), seed=10), {}, 2),
    "sides_child0": (lambda: C.tree_model(T7, (5, 9, 7, 9, 5, 4, 6), "dense", seed=11, sides="child0"), {}, 0),
    "sides_child1": (lambda: C.tree_model(T7, (5, 9, 7, 9, 5, 4, 6), "dense", seed=12, sides="child1"), {}, 0),
    "sides_mixed": (lambda: C.tree_model(T7, (5, 9, 7, 9, 5, 4, 6), "dense", seed=13, sides="mixed"), {}, 0),
    "rect_both_forms_and_widths": (lambda: C.rect_case(), {}, 0),
    "fan1": (lambda: C.fan_case(1), {}, 0),
    "fan2": (lambda: C.fan_case(2), {}, 0),
    "fan8": (lambda: C.fan_case(8), {}, 0),
    "fan9": (lambda: C.fan_case(9), {}, 0),
    "fan40": (lambda: C.fan_case(40), {}, 2),
    "ties_dense": (lambda: C.tree_model(T7, (6,) * 7, "dense", seed=16, ints=True), {}, 0),
    "ties_potts": (lambda: C.tree_model(T7, (6,) * 7, "potts", seed=17, ints=True), {}, 0),
    "ties_diff": (lambda: C.tree_model(T7, (6,) * 7, "diff", seed=18, ints=True), {}, 0),
    "inf_tables": (lambda: (PC.inf_case()[0], _inf_groups()), {}, 0),
    "all_inf_root": (lambda: (PC.all_inf_case()[0], M.forests_from_paths(PC.all_inf_case()[1])), {}, 0),
    "all_inf_leaf": (lambda: (PC.all_inf_case()[0], [(np.asarray([0, 1, 2], np.int32), np.asarray([-1, 0, 1], np.int32))]), {}, 0),
}


@pytest.mark.parametrize("name", sorted(KINDS))
def test_moves_match_the_statement(name):
    make, kw, passes = KINDS[name]
    m, groups = make()
    if name.startswith("ties") or name.startswith("all_inf"):      # the duals are the costs themselves (zero messages): quantised, ties everywhere
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
    if name.startswith("all_inf"):
        assert got[2, 0] == 0
    if name == "rect_both_forms_and_widths":
        # rows: sum of d_parent = 9 + 300 + 9 + 5 + 5; back-pointers: 300 -> 2 bytes x 9, 40 -> 300, 5 -> 9, 7 -> 5, then 257 -> 2 x 5 at an even byte
        fs = e.forest_set(groups)
        assert fs.scratch_bytes == 8 * (9 + 300 + 9 + 5 + 5) + (2 * 9 + 300 + 9 + 5 + 2 * 5) and fs.max_height == 2
        fs.close()
    e.close()


@pytest.mark.parametrize("L", [1, 2, 3, 8, 31, 32, 33, 64, 65, 130, 256, 257, 512])
def test_label_counts(L):
    """a root, two children and a grandchild of L labels, an off-tree neighbour each; random duals (passes on more than 256 labels are
    beyond the sweep kernels).  512 labels: DIFF factors (a dense table would be 2 MB each)"""
    m, groups = C.labels_case(L)
    e = _engine(m, 0, L)
    _check_moves(e, m, groups, C.random_primal(m, L), rounds=1, what="L=%d" % L)
    fs = e.forest_set(groups)
    assert fs.scratch_bytes == 3 * L * (9 if L <= 256 else 10)
    fs.close()
    e.close()


@pytest.mark.parametrize("root", ["hub", "leaf"])
def test_star(root):
    m = DC.star()                          # hub 35 with 70 leaves on alternating sides
    leaves = [v for v in range(71) if v != 35]
    par = [-1] + [35] * 70 if root == "hub" else [0, -1] + [35] * 69
    groups = [(np.asarray([35] + leaves, np.int32), np.asarray(par, np.int32))]
    e = _engine(m, 2)
    _check_moves(e, m, groups, C.random_primal(m, 1), rounds=1, what="star " + root)
    e.close()


def test_300_height_levels_equal_the_statement_and_the_path_move():
    m, path_groups = PC.long_case()
    groups = M.forests_from_paths(path_groups)
    e = _engine(m, 2)
    start = C.random_primal(m, 7)
    got = _check_moves(e, m, groups, start, rounds=1, what="length300")
    fs = e.forest_set(groups)
    assert fs.max_height == 299 and fs.n_trees == 2
    fs.close()
    e.upload_primal(start)
    ps = e.path_set(path_groups)
    ps.move(1)
    assert np.array_equal(e.download_primal(), got)
    ps.close(); e.close()


GRAPHS = {"grid7x6_row": lambda: PC.grid(7, 6, 5, "row_major"), "grid7x6_colour": lambda: PC.grid(7, 6, 5, "colour_major"),
          "grid12x9_row": lambda: PC.grid(12, 9, 5, "row_major"), "grid12x9_colour": lambda: PC.grid(12, 9, 5, "colour_major"),
          "random_graph": DC.random_graph}


@pytest.mark.parametrize("name,rounds", [("grid7x6_row", 3), ("grid7x6_colour", 1), ("grid12x9_row", 2), ("grid12x9_colour", 3), ("random_graph", 1), ("random_graph", 3)])
def test_grids_and_graphs_with_the_suggested_cover(name, rounds):
    m = GRAPHS[name]()
    e = _engine(m, 3)
    e.decode_primal(0, 0)
    start = e.download_primal()
    groups = E.Plan(m).suggest_forests()
    got = _check_moves(e, m, groups, start, rounds=rounds, what=(name, rounds))
    # state: evaluate_primal prices the device's labels; a read-out agrees; the energy did not rise and stays above the bound
    assert e.check_primal_consistency()
    cost, want, before = e.evaluate_primal(), C.energy(m, got), C.energy(m, start)
    assert abs(cost - want) <= 1e-9 * max(1.0, abs(want))
    assert want <= before + 1e-9 * max(1.0, abs(before)) and cost >= e.lower_bound() - 1e-9 * max(1.0, abs(cost))
    unaries, _ = C.structure(m)
    r = e.readout()
    assert np.array_equal(r.labels(), got[unaries, 0])
    r.close()
    e.close()


def test_an_unset_neighbour_is_clamped():
    """the off-tree neighbours hold no label (the dimension, as after an upload): they count with their LAST label"""
    m, groups = C.tree_model(T7, (5, 9, 7, 9, 5, 4, 6), "dense", seed=21)
    e = _engine(m, 0, 5)
    unset = e.download_primal()
    assert np.array_equal(unset[:14, 0], m.f_dim0[:14])
    got = _check_moves(e, m, groups[:1], unset, rounds=1, what="unset")
    assert np.all(got[:7, 0] < m.f_dim0[:7]) and np.array_equal(got[7:14], unset[7:14])
    stray = unset.copy()                   # a negative stray label counts as label 0
    stray[7:14, 0] = -7
    _check_moves(e, m, groups[:1], stray, rounds=1, what="stray")
    e.close()


def test_a_model_the_rounding_code_refuses():
    """the Potts grid of c5_model with labeling-list factors beside it: the labels live in the array of unset labels and are read
    through a read-out (as in the path-move tests)"""
    H, W, L = 5, 4, 4
    m5 = S.c5_model(H, W, L, 12, 6, 3, seed=2, window=12)
    mg = S.grid_model(H, W, L, pairwise="potts", order="colour_major", seed=2)
    groups = E.Plan(mg).suggest_forests()
    e = _engine(m5, 2)
    with pytest.raises(E.EngineError):
        e.download_primal()
    duals = e.download_duals()[:mg.dual_data.shape[0]]
    unset = np.stack([mg.f_dim0, np.where(mg.f_kind == M.F_VECTOR, 0, mg.f_dim1)], 1).astype(np.int32)
    trace = []
    C.forest_moves_reference(mg, duals, unset, groups, rounds=2, trace=trace)
    fs = e.forest_set(groups)
    r = e.readout(np.arange(H * W))
    fs.move(2)
    assert np.array_equal(r.labels(), trace[-1][:H * W, 0])
    fs.close(); r.close(); e.close()


def test_a_move_writes_labels_only():
    for make, kw in ((lambda: (PC.grid(9, 7, 8, "colour_major"), None), {}), (lambda: C.tree_model(T7, (13,) * 7, "dense", seed=3), {"rows_layout": True}),
                     (lambda: C.tree_model(T7, (13,) * 7, ("dense", "potts", "shared", "diff", "diff_banded", "dense"), seed=10), {})):
        m, groups = make()
        if groups is None:
            groups = E.Plan(m).suggest_forests()
        e = _engine(m, 3, **kw)
        e.enable_kernel_timing(True)
        e.compute_pass(1)
        e.upload_primal(C.random_primal(m, 3))
        built = e.schedules_built()
        fs = e.forest_set(groups)
        assert e.schedules_built() == built + 1                # the create is counted once
        lb0 = e.lower_bound()
        d0, f0, kt0 = e.download_duals(), e.factor_lower_bounds(), e.kernel_timing()
        lb0b, rec0b = e.lower_bound(), e.lower_bound_recomputed()
        fs.move(1); fs.move(3)
        assert e.schedules_built() == built + 1                # a move plans nothing
        lb1, rec1 = e.lower_bound(), e.lower_bound_recomputed()
        d1, f1, kt1 = e.download_duals(), e.factor_lower_bounds(), e.kernel_timing()
        assert d0.tobytes() == d1.tobytes() and f0.tobytes() == f1.tobytes() and kt0 == kt1
        assert np.float64(lb0).tobytes() == np.float64(lb0b).tobytes() == np.float64(lb1).tobytes()
        assert rec1 <= rec0b                                   # the moves made no tracked bound stale
        f = _engine(m, 3, **kw)                                # a pass afterwards continues as on an engine that never moved
        f.compute_pass(1)
        e.compute_pass(1); f.compute_pass(1)
        assert np.array_equal(e.download_duals(), f.download_duals())
        fs.close()
        e.close(); f.close()


def test_a_move_runs_on_the_costs_of_the_moment():
    import recost_cases as RC
    A = RC.grid(9, 7, 8)
    B = RC.recost(A, 77)
    groups = E.Plan(A).suggest_forests()
    e = _engine(A, 2)
    fs = e.forest_set(groups)
    built = e.schedules_built()

    def check(m, what):
        start = C.random_primal(m, 4)
        e.upload_primal(start)
        fs.move(2)
        got, want = e.download_primal(), C.forest_moves_reference(m, e.download_duals(), start, groups, rounds=2)
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
    fs.close(); e.close()
    # pool values
    m, groups = C.tree_model(T7, (13, 7, 13, 7, 13, 7, 13), "shared", seed=7)
    e = _engine(m, 2)
    fs = e.forest_set(groups)
    m2 = m.with_pool(m.sh_data * 0.5 + 0.25)
    e.upload_shared_pool(m2.sh_data)
    start = C.random_primal(m2, 6)
    e.upload_primal(start)
    fs.move(1)
    assert np.array_equal(e.download_primal(), C.forest_moves_reference(m2, e.download_duals(), start, groups))
    fs.close(); e.close()
    # moved windows: the shifts and the duals of the moment
    m, groups = C.diff_shift_tree()
    e = _engine(m, 2)
    fs = e.forest_set(groups)
    ws = e.window_set()
    delta = np.random.default_rng(8).integers(-3, 4, ws.n)
    m2, d2 = M.move_windows(m, e.download_duals(), None, delta)
    ws.move(delta)
    assert np.array_equal(e.download_duals(), d2)
    start = C.random_primal(m2, 9)
    e.upload_primal(start)
    fs.move(2)
    assert np.array_equal(e.download_primal(), C.forest_moves_reference(m2, d2, start, groups, rounds=2))
    ws.close(); fs.close(); e.close()


def test_a_move_settles_passes_that_ran_ahead(monkeypatch):
    """as tests/test_path_moves_gpu.py: with speculation on the device is passes ahead of the caller; the move first settles"""
    monkeypatch.setenv("LPMP_ROT_BANDS", "6")
    H, W = 40, 36
    m = S.grid_model(H, W, 32, order="colour_major", seed=6)
    groups = M.forests_from_paths(S.grid_paths(H, W, "colour_major")[:1])
    e, f = E.Engine(0), E.Engine(0)
    for x in (e, f):
        x.upload(m); x.set_reparametrization(ANISO)
        x.lower_bound()
    e.set_speculation(8)
    for k in range(4):
        e.compute_pass(1); f.compute_pass(1)
    st = e.speculation_stats()
    assert st["batches"] == 2 and st["passes_launched"] == 6 and st["rollbacks"] == 0, st
    fe, ff = e.forest_set(groups), f.forest_set(groups)
    start = C.random_primal(m, 11)
    fe.move(1)                                                  # settles; the labels are still unset here
    assert e.speculation_stats()["rollbacks"] == 1
    assert np.array_equal(e.download_duals(), f.download_duals())
    for x, fs in ((e, fe), (f, ff)):
        x.upload_primal(start); fs.move(1)
    got = e.download_primal()
    assert np.array_equal(got, f.download_primal())
    assert np.array_equal(got, PC.path_moves_reference(m, e.download_duals(), start, S.grid_paths(H, W, "colour_major")[:1]))
    fe.close(); ff.close(); e.close(); f.close()


def test_error_returns_stale_and_empty_sets_and_the_lp_mirror():
    m, groups = C.tree_model((-1, 0, 0), (5, 6, 4), "dense", seed=15)
    e = E.Engine(0)
    with pytest.raises(E.EngineError) as ei:
        e.forest_set(groups)
    assert ei.value.code == ERR_STATE
    e.upload(m)
    fs = e.forest_set(groups)
    with pytest.raises(E.EngineError) as ei:
        fs.move(-1)
    assert ei.value.code == ERR_INVALID
    with pytest.raises(E.EngineError) as ei:
        e.forest_set([([1, 2], [-1, 1])])
    assert ei.value.code == ERR_INVALID and "no pairwise factor joins" in str(ei.value)
    start = C.random_primal(m, 1)
    e.upload_primal(start)
    fs.move(0)                                                  # rounds = 0: nothing moves
    assert np.array_equal(e.download_primal(), start)
    for empty in ([], [([], []), ([], [])]):
        es = e.forest_set(empty)
        assert (es.n_groups, es.n_trees, es.max_height, es.scratch_bytes) == (len(empty), 0, 0, 0)
        es.move(3)
        assert np.array_equal(e.download_primal(), start)
        es.close()
    fs.move(1)                                                  # no weights needed: a move reads duals, constants and labels
    assert np.array_equal(e.download_primal(), C.forest_moves_reference(m, m.dual_data, start, groups))
    e.upload(m)                                                 # a stale set
    with pytest.raises(E.EngineError) as ei:
        fs.move(1)
    assert ei.value.code == ERR_STATE
    fs.close(); fs.close()
    mc = S.multicut_triangle_model(6, 4, seed=1)
    e.upload(mc)
    with pytest.raises(E.EngineError) as ei:
        e.forest_set([([0], [-1])])
    assert ei.value.code == ERR_UNSUPPORTED and "factor 0 " in str(ei.value)
    e.close()
    # LP mirror: the README quick-start model (optimum 1.0 at labels (0, 0) or (1, 1)); the suggested cover is the one tree u1 - u2
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
    for groups in (None, [([u1, u2], [u2, -1])]):
        cost = lp.forest_moves(groups, rounds=1)
        pr = lp.primal()
        assert cost == 1.0 and lp.CheckPrimalConsistency() and list(pr[p]) == [pr[u1, 0], pr[u2, 0]] == [0, 0]


# ---- far offsets: the live model behind 2^31 elements of padding (tests/far_offset_cases.py) ------------------------------------
def test_a_forest_behind_far_offsets():
    """the DIFF_SHIFT tree behind 32 768 isolated 1 x 65 536 dense factors: every dual and constant offset of the node and link
    records lies past 2^31 elements.  Labels against the statement on the small model"""
    import torch
    import far_offset_cases as F
    need, free = F.FarBuffers.bytes_needed("P31"), torch.cuda.mem_get_info()[0]
    assert free >= need + F.GIB, "the device reports %.1f GiB free, the padding needs %.1f GiB" % (free / F.GIB, need / F.GIB)
    bufs = F.FarBuffers("P31")
    try:
        m, groups = C.diff_shift_tree()
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
        fs = e.forest_set([(un + n_pad, np.where(par == -1, -1, par + n_pad)) for un, par in groups])
        fs.move(2)
        got = e.download_primal()
        want = C.forest_moves_reference(m, duals, start, groups, rounds=2)
        assert np.array_equal(got[n_pad:], want), _differ(got[n_pad:], want)
        assert np.array_equal(got[:n_pad], pr[:n_pad])
        e.synchronize()
        assert np.array_equal(bufs.dual_tail(), duals) and bufs.dual_padding_nonzero() == 0
        fs.close(); e.close()
        bufs.reset()
    finally:
        bufs.const = bufs.dual = None
        torch.cuda.empty_cache()
