"""Path moves, host side: the numpy statement of the rule (tests/path_moves_cases.py) against brute force, against the
decode's refinement rule and against itself over paths, groups and rounds on duals of the CPU oracle; the planner's checks
(lpmp_plan_path_info) with every refusal; the ABI.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import decode_cases as DC
import path_moves_cases as C

ANISO = M.REPAM_ANISOTROPIC
ERR_INVALID, ERR_UNSUPPORTED = -1, -2
NEW_INT = ("lpmp_path_set_create", "lpmp_path_moves", "lpmp_plan_path_info")
NEW_OTHER = ("lpmp_path_set_destroy", "lpmp_path_set_n_groups", "lpmp_path_set_n_paths", "lpmp_path_set_longest", "lpmp_path_set_scratch_bytes")


def _duals(m, passes):
    o = Oracle(m.expand_shared().expand_diff())          # (the oracle's kinds; same factors, same dual layout)
    o.set_reparametrization(ANISO)
    if passes:
        o.ComputePass(passes)
    return o


# ---- the statement against brute force ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 2])
def test_a_path_over_a_whole_chain_reaches_the_optimum_from_any_labelling(passes):
    for seed in range(20):
        m = DC.chain(seed)
        best = C.brute_force(m)
        duals = _duals(m, passes).duals()
        for start in range(3):
            pr = C.path_moves_reference(m, duals, C.random_primal(m, 100 * seed + start), [[list(range(6))]])
            e = C.energy(m, pr)
            assert abs(e - best) <= 1e-12 * max(1.0, abs(best)), (seed, start, e, best)


@pytest.mark.parametrize("kind", ["dense", "potts", "shared", "diff"])
def test_a_move_equals_exhaustive_search_over_the_path(kind):
    """the 5-variable graph of decode_cases.small_graph (edges 0-1, 1-2, 3-2, 0-3, 0-2, 4-2): every chordless path of it.  Slack
    1e-9 * max(1, |E|): the move minimises the energy written with theta + sum m, the search the original one; the two differ by
    the rounding of some tens of terms of magnitude <= 3"""
    paths = [[1, 2, 4], [1, 0, 3], [4, 2, 3], [0, 1], [3, 2], [2], [4, 2, 1]]
    for seed in (1, 2):
        m = DC.small_graph(3, seed, kind)
        for passes in (0, 3):
            duals = _duals(m, passes).duals()
            for k, path in enumerate(paths):
                start = C.random_primal(m, seed * 10 + k)
                pr = C.path_moves_reference(m, duals, start, [[path]])
                others = [u for u in range(5) if u not in path]
                assert np.array_equal(pr[others], start[others])
                e, want = C.energy(m, pr), C.best_over_path(m, start, path)
                assert abs(e - want) <= 1e-9 * max(1.0, abs(want)), (kind, seed, passes, path, e, want)


def test_paths_of_one_member_are_the_refinement_sweep_of_the_decode():
    for m in (DC.grid(7, 6, 4, "colour_major"), DC.random_graph(), DC.mixed_case(), DC.duplicate_edges()):
        o = _duals(m, 3)
        sweeps = []
        DC.decode_reference(m, o.duals(), o.order(0), refine=2, sweeps_out=sweeps)
        pi = DC.decode_order(m, o.order(0))
        got = C.path_moves_reference(m, o.duals(), sweeps[0], [[[u]] for u in pi], rounds=1)
        assert np.array_equal(got, sweeps[1])
        got = C.path_moves_reference(m, o.duals(), sweeps[0], [[[u]] for u in pi], rounds=2)
        assert np.array_equal(got, sweeps[2])


@pytest.mark.parametrize("kind", ["random", "truncated"])
@pytest.mark.parametrize("order", ["row_major", "colour_major"])
def test_energy_never_rises_over_paths_groups_and_rounds(kind, order):
    """The table of DESIGN.md 8 with the two new columns.  Guaranteed and asserted: the energy does not rise over any path (so over
    any group and round) and stays at or above the bound.  Slack 1e-9 * max(1, |E|), the argument of
    test_energy_does_not_rise_over_refinement_sweeps: sums of ~1700 terms of magnitude <= 1."""
    m = C.table_grid(kind, order)
    groups = S.grid_paths(24, 24, order)
    o = _duals(m, 0)
    done = 0
    for passes in (5, 50):
        o.ComputePass(passes - done)
        done = passes
        duals = o.duals()
        sweeps = []
        DC.decode_reference(m, duals, o.order(0), refine=3, sweeps_out=sweeps)
        start = sweeps[0]
        en = [C.energy(m, start)]

        def after_path(label):
            en.append(C.energy(m, C.labels_to_primal(m, label)))

        trace = []
        C.path_moves_reference(m, duals, start, groups, rounds=3, trace=trace, per_path=after_path)
        slack = 1e-9 * max(1.0, abs(en[0]))
        assert len(en) == 1 + 3 * 48 and len(trace) == 12
        for a, b in zip(en, en[1:]):
            assert b <= a + slack, (a, b)
        rounds = [C.energy(m, trace[4 * r + 3]) for r in range(3)]
        assert abs(rounds[2] - en[-1]) <= slack
        lb = o.LowerBound()
        assert en[-1] >= lb - slack
        print("%s, %s, %d passes | bound %.2f | decode %.2f | decode + 3 ICM sweeps %.2f | + 1 round of path moves %.2f | + 2 rounds %.2f | + 3 rounds %.2f"
              % (kind, order, passes, lb, en[0], C.energy(m, sweeps[3]), rounds[0], rounds[1], rounds[2]))


# ---- lpmp_plan_path_info -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["row_major", "colour_major"])
def test_counts_on_grids(order):
    H, W = 7, 6
    m = C.grid(H, W, 4, order)
    groups = S.grid_paths(H, W, order)
    assert [len(g) for g in groups] == [4, 3, 3, 3] and all(len(p) == W for g in groups[:2] for p in g) and all(len(p) == H for g in groups[2:] for p in g)
    n_edges = H * (W - 1) + W * (H - 1)
    # every edge is a path edge of its row or column, and an off-path link of both its unaries in the other pair of groups
    assert E.Plan(m).path_info(groups) == {"n_paths": H + W, "n_path_edges": n_edges, "n_off_path_links": 2 * n_edges}
    assert E.Plan(m).path_info(groups[:1]) == {"n_paths": 4, "n_path_edges": 4 * (W - 1), "n_off_path_links": W + 2 * W + 2 * W + W}      # (rows 0 and 6 have one row next to them)
    assert E.Plan(m).path_info([]) == {"n_paths": 0, "n_path_edges": 0, "n_off_path_links": 0}
    assert E.Plan(m).path_info([[], []]) == {"n_paths": 0, "n_path_edges": 0, "n_off_path_links": 0}
    # the statement finds the same edges
    _, links = C.structure(m)
    assert sum(len(C.path_edges(p, links)) for g in groups for p in g) == n_edges


def test_counts_on_a_star_and_next_to_parallel_edges():
    m = DC.star()              # hub 35, leaves 0 .. 70 without it
    p = E.Plan(m)
    assert p.path_info([[[0, 35, 1]], [[2, 35, 70]], [[3], [4]], [[35]]]) == {"n_paths": 5, "n_path_edges": 4, "n_off_path_links": 68 + 68 + 1 + 1 + 70}
    why = _refusal(m, [[[3], [35]]], ERR_INVALID)       # (a leaf and the hub are neighbours: not in one group)
    assert "two paths of group 0" in why
    m = DC.duplicate_edges()   # variables 0 and 1 share three pairwise factors, 1 and 2 one
    p = E.Plan(m)
    assert p.path_info([[[1, 2]], [[2, 1]], [[0], [2]]]) == {"n_paths": 4, "n_path_edges": 2, "n_off_path_links": 3 + 3 + 3 + 1}


def _refusal(m, groups, code):
    with pytest.raises(E.EngineError) as ei:
        E.Plan(m).path_info(groups)
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


def _raw_info(m, group_off, path_off, unaries):
    p = E.Plan(m)
    go, po, un = np.asarray(group_off, np.int64), np.asarray(path_off, np.int64), np.asarray(unaries + [0], np.int32)
    buf = ctypes.create_string_buffer(512)
    rc = p.L.lpmp_plan_path_info(p.h, go.shape[0] - 1, go.ctypes.data, po.ctypes.data, un.ctypes.data, None, None, None, buf, 512)
    return rc, buf.value.decode()


def test_invalid_sets_name_the_entry():
    H, W = 4, 5
    m = C.grid(H, W, 3, "row_major")           # unary of (r, c): r * W + c; pairwise factors from H * W on
    row = lambda r: [r * W + c for c in range(W)]
    # offsets
    rc, why = _raw_info(m, [0, 2, 1], [0, 1, 2], [0, 2])
    assert rc == ERR_INVALID and "group_off" in why and "group 1" in why
    rc, why = _raw_info(m, [0, 2], [0, 2, 1], [0, 1])
    assert rc == ERR_INVALID and "path_off" in why and "path 1" in why
    rc, why = _raw_info(m, [0, 2], [0, 1, 1], [0])
    assert rc == ERR_INVALID and "path 1" in why and "at least one member" in why
    rc, why = _raw_info(m, [1, 2], [0, 1, 2], [0, 2])
    assert rc == ERR_INVALID and "group_off[0]" in why
    rc, why = _raw_info(m, [0, 1], [0, 1], [0])
    assert rc == 0 and why == ""
    # indices and kinds
    why = _refusal(m, [[[0, 1, H * W + 100000]]], ERR_INVALID)
    assert "out of range" in why and "entry 2" in why
    why = _refusal(m, [[[0, -1]]], ERR_INVALID)
    assert "out of range" in why and "entry 1" in why
    why = _refusal(m, [[[0, 1], [H * W]]], ERR_INVALID)
    assert "factor %d " % (H * W) in why and "entry 2" in why and "not a VECTOR" in why
    # a unary twice in one group: in one path, in two paths; in two GROUPS it is fine
    why = _refusal(m, [[[0, 1, 0]]], ERR_INVALID)
    assert "factor 0 " in why and "entry 2" in why and "twice in group 0" in why and "entry 0" in why
    why = _refusal(m, [[row(0)], [row(2), [W, 2 * W]]], ERR_INVALID)
    assert "factor %d " % (2 * W) in why and "entry %d" % (2 * W + 1) in why and "twice in group 1" in why
    assert E.Plan(m).path_info([[row(0)], [row(0)]])["n_paths"] == 2
    # consecutive members without a pairwise factor
    why = _refusal(m, [[[0, 1, W + 2]]], ERR_INVALID)
    assert "no pairwise factor joins" in why and "factor 1 (entry 1)" in why and "factor %d (entry 2)" % (W + 2) in why
    # a ring: the four unaries of a grid cell, the last joined to the first
    why = _refusal(m, [[[0, 1, W + 1, W]]], ERR_INVALID)
    assert "non-consecutive members of path 0" in why and "ring" in why and "entry 0" in why and "entry 3" in why
    # ... and a chord further inside a path
    why = _refusal(m, [[[0, 1, W + 1, W, 2 * W]]], ERR_INVALID)
    assert "non-consecutive members of path 0" in why
    # two adjacent rows in one group
    why = _refusal(m, [[row(0), row(1)]], ERR_INVALID)
    assert "two paths of group 0" in why and "factor 0 (entry 0)" in why and "factor %d (entry %d)" % (W, W) in why
    # the parallel edges of duplicate_edges: variables 0 and 1 are joined by three pairwise factors
    why = _refusal(DC.duplicate_edges(), [[[2, 1, 0]]], ERR_INVALID)
    assert "more than one pairwise factor" in why and "factor 1 (entry 1)" in why and "factor 0 (entry 2)" in why
    why = _refusal(DC.duplicate_edges(), [[[0, 1]]], ERR_INVALID)
    assert "more than one pairwise factor" in why


def test_unsupported_sets_name_the_lowest_listed_unary():
    # a labeling message next to a listed unary
    mc = S.multicut_triangle_model(6, 4, seed=1)
    why = _refusal(mc, [[[3], [1]], [[2]]], ERR_UNSUPPORTED)
    assert "factor 1 " in why and "not a unary-pairwise message" in why
    # ... but only next to a LISTED one: the Potts grid of c5_model with labeling-list factors elsewhere
    m5 = S.c5_model(5, 4, 4, 12, 6, 3, seed=2, window=12)
    assert E.Plan(m5).path_info(S.grid_paths(5, 4, "colour_major"))["n_paths"] == 9
    ev = min(int(m5.m_left[k]) for k in range(m5.n_messages) if m5.mtypes[int(m5.m_type[k])].kind == M.M_LABELING)
    why = _refusal(m5, [[[0]], [[ev]]], ERR_UNSUPPORTED)
    assert "factor %d " % ev in why and "not a unary-pairwise message" in why
    r = np.random.default_rng(0)
    un = [r.random(3) for _ in range(4)]
    T = lambda: ("dense", r.random((3, 3)))
    edges = [(0, 1, T()), (1, 2, T()), (2, 3, T())]          # pairwise factors 4, 5, 6
    both = [(0, 0, 0), (1, 1, 0), (0, 1, 1), (1, 2, 1), (0, 2, 2), (1, 3, 2)]
    assert E.Plan(C.build_model(un, edges, both)).path_info([[[0, 1, 2, 3]]])["n_path_edges"] == 3
    # factor 5 has no unary on side 1: unary 1 is the lowest listed one next to it; unlisted, nobody minds
    lame = C.build_model(un, edges, [x for x in both if x != (1, 2, 1)])
    why = _refusal(lame, [[[3], [1]], [[0]]], ERR_UNSUPPORTED)
    assert "factor 1 " in why and "pairwise factor 5" in why and "exactly one unary on each side" in why
    assert E.Plan(lame).path_info([[[3], [0]]])["n_paths"] == 2
    # two unaries on side 0 of factor 6, one unary on both sides of factor 4
    why = _refusal(C.build_model(un, edges, both + [(0, 0, 2)]), [[[3]]], ERR_UNSUPPORTED)
    assert "factor 3 " in why and "pairwise factor 6" in why
    why = _refusal(C.build_model(un, edges, [(0, 1, 0), (1, 1, 0)] + both[2:]), [[[2, 1]]], ERR_UNSUPPORTED)
    assert "factor 1 " in why and "pairwise factor 4" in why
    # more than 512 labels
    big = C.build_model([r.random(513), r.random(2), r.random(512)], [(0, 1, ("dense", r.random((513, 2)))), (2, 1, ("dense", r.random((512, 2))))])
    why = _refusal(big, [[[2, 1, 0]]], ERR_UNSUPPORTED)
    assert "factor 0 " in why and "513 labels" in why
    assert E.Plan(big).path_info([[[2, 1]]])["n_path_edges"] == 1


def test_grid_paths():
    for order in ("row_major", "colour_major"):
        var = S.grid_variable_order(3, 5, order)
        g = S.grid_paths(3, 5, order)
        assert g[0] == [var[0].tolist(), var[2].tolist()] and g[1] == [var[1].tolist()]
        assert g[2] == [var[:, 0].tolist(), var[:, 2].tolist(), var[:, 4].tolist()] and g[3] == [var[:, 1].tolist(), var[:, 3].tolist()]
    assert S.grid_paths(1, 2, "row_major") == [[[0, 1]], [], [[0]], [[1]]]


def test_abi_declares_and_exports_the_calls():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "lpmp_engine.h")).read()
    L = E.lib()
    assert "typedef struct lpmp_path_set lpmp_path_set;" in hdr
    for fn in NEW_INT:
        assert re.search(r"\bint %s\(" % fn, hdr) and fn in E.EXPORTS and hasattr(L, fn)
    assert re.search(r"\bvoid lpmp_path_set_destroy\(", hdr)
    for fn in NEW_OTHER[1:]:
        assert re.search(r"\bint64_t %s\(const lpmp_path_set\*" % fn, hdr)
    for fn in NEW_OTHER:
        assert fn in E.EXPORTS and hasattr(L, fn)
