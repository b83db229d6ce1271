"""Forest moves, host side: the numpy statement of the rule (tests/forest_moves_cases.py) against the statement of the
path moves, against brute force on tree models and against itself over groups and rounds on duals of the CPU oracle; the planner's
checks (lpmp_plan_forest_info) with every refusal; the suggested cover (lpmp_plan_suggest_forests); the ABI.  No GPU."""
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
import forest_moves_cases as C
import path_moves_cases as PC

ANISO = M.REPAM_ANISOTROPIC
ERR_INVALID, ERR_UNSUPPORTED = -1, -2
NEW_INT = ("lpmp_forest_set_create", "lpmp_forest_moves", "lpmp_plan_forest_info", "lpmp_plan_suggest_forests")
NEW_OTHER = ("lpmp_forest_set_destroy", "lpmp_forest_set_n_groups", "lpmp_forest_set_n_trees", "lpmp_forest_set_max_height", "lpmp_forest_set_scratch_bytes")


def _oracle(m, passes):
    o = Oracle(m.expand_shared().expand_diff())          # (the oracle's kinds; same factors, same dual layout)
    o.set_reparametrization(ANISO)
    if passes:
        o.ComputePass(passes)
    return o


def _dual_sets(m, seed=0):
    """the duals after 0 and 2 oracle passes, and random numbers (the rule reads any duals)"""
    return [_oracle(m, 0).duals(), _oracle(m, 2).duals(), np.random.default_rng(seed).random(m.dual_data.shape[0])]


# ---- against path moves ------------------------------------------------------------------------------------------------------------
def _same_as_path_moves(m, path_groups, what):
    groups = M.forests_from_paths(path_groups)
    assert C.as_paths(groups) == [[[int(u) for u in p] for p in g] for g in path_groups]
    for k, duals in enumerate(_dual_sets(m, 5)):
        start = C.random_primal(m, 3 + k)
        want, got = [], []
        PC.path_moves_reference(m, duals, start, path_groups, rounds=2, trace=want)
        C.forest_moves_reference(m, duals, start, groups, rounds=2, trace=got)
        assert len(want) == len(got) == 2 * len(path_groups)
        for i, (a, b) in enumerate(zip(want, got)):
            assert np.array_equal(a, b), (what, k, i)


@pytest.mark.parametrize("kind", ["dense", "potts", "shared", "diff", "diff_banded"])
def test_path_shaped_forests_equal_path_moves_on_ladders(kind):
    dims = (6, 6, 6, 6) if kind in ("potts", "diff_banded") else (5, 9, 7, 4)
    for flip in ("alternate", "none", "all"):
        m, path_groups = PC.ladder(dims, kind, seed=3, flip=flip)
        _same_as_path_moves(m, path_groups, (kind, flip))
    m, path_groups = PC.ladder((6, 6, 6, 6), "dense" if kind == "diff_banded" else kind, seed=16, ints=True)      # ties
    _same_as_path_moves(m, path_groups, (kind, "ints"))


def test_path_shaped_forests_equal_path_moves_on_diff_shift_and_mixed_kinds():
    _same_as_path_moves(*PC.diff_shift_case(), "diff_shift")
    _same_as_path_moves(*PC.mixed_path_case(), "mixed")


@pytest.mark.parametrize("order", ["row_major", "colour_major"])
@pytest.mark.parametrize("shape", [(7, 6), (12, 9)])
def test_path_shaped_forests_equal_path_moves_on_grids(shape, order):
    H, W = shape
    _same_as_path_moves(PC.grid(H, W, 5, order), S.grid_paths(H, W, order), (shape, order))


# ---- tree models: the optimum ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 2])
def test_a_forest_that_is_the_whole_tree_model_reaches_the_optimum(passes):
    sizes = set()
    cases = [C.random_tree(s) for s in range(16)] + [C.tiny_tree(s) for s in range(4)]
    for i, (m, parents) in enumerate(cases):
        sizes.add(len(parents))
        if len(parents) >= 4:      # a node with three children, one on side 0 and one on side 1 of its edge
            _, links = C.structure(m)
            assert parents[:4] == [-1, 0, 0, 0] and {s for _, s, w in links[0] if w in (1, 2)} == {0, 1}
        best = C.brute_force(m)
        duals = _oracle(m, passes).duals()
        group = C.whole_tree_group(m, parents)
        for start in range(3):
            pr = C.forest_moves_reference(m, duals, C.random_primal(m, 100 * i + start), group)
            e = C.energy(m, pr)
            # the move minimises the energy written with theta + sum m; the two differ by the rounding of < 30 terms below 3
            assert abs(e - best) <= 1e-12 * max(1.0, abs(best)), (i, start, e, best)
        # re-rooted anywhere, the optimum again
        k = len(parents)
        nb = {v: [q for q in (parents[v],) if q >= 0] + [c for c in range(k) if parents[c] == v] for v in range(k)}
        root = k - 1
        par, stack = {root: -1}, [root]
        while stack:
            v = stack.pop()
            for w in nb[v]:
                if w not in par:
                    par[w] = v
                    stack.append(w)
        pr = C.forest_moves_reference(m, duals, C.random_primal(m, i), C.whole_tree_group(m, [par[v] for v in range(k)]))
        assert abs(C.energy(m, pr) - best) <= 1e-12 * max(1.0, abs(best))
    assert sizes == {2, 3, 4, 5, 6, 7}


def test_single_nodes_are_one_step_of_the_refinement_sweep():
    m = DC.random_graph()
    o = _oracle(m, 3)
    sweeps = []
    DC.decode_reference(m, o.duals(), o.order(0), refine=1, sweeps_out=sweeps)
    pi = DC.decode_order(m, o.order(0))
    got = C.forest_moves_reference(m, o.duals(), sweeps[0], [([u], [-1]) for u in pi])
    assert np.array_equal(got, sweeps[1])


# ---- energy on cyclic graphs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random_graph", "thinned_grid", "star"])
def test_energy_never_rises_over_the_groups_of_the_suggested_cover(name):
    """Guaranteed and asserted: the energy does not rise over any group of three rounds and stays at or above the oracle's bound.
    Slack 1e-9 * max(1, |E|): sums of some hundreds of terms of magnitude <= 1, as in the path-move tests."""
    m = {"random_graph": DC.random_graph, "thinned_grid": C.thinned_grid, "star": DC.star}[name]()
    groups = E.Plan(m).suggest_forests()
    o = _oracle(m, 0)
    done = 0
    for passes in (0, 2, 20):
        o.ComputePass(passes - done)
        done = passes
        start = C.random_primal(m, passes) if passes == 0 else DC.decode_reference(m, o.duals(), o.order(0))
        trace = []
        C.forest_moves_reference(m, o.duals(), start, groups, rounds=3, trace=trace)
        en = [C.energy(m, start)] + [C.energy(m, t) for t in trace]
        slack = 1e-9 * max(1.0, abs(en[0]))
        assert len(en) == 1 + 3 * len(groups)
        for a, b in zip(en, en[1:]):
            assert b <= a + slack, (name, passes, a, b)
        assert en[-1] >= o.LowerBound() - slack
        print("%s, %d passes, %d groups | bound %.3f | start %.3f | after 1, 2, 3 rounds %s"
              % (name, passes, len(groups), o.LowerBound(), en[0], ["%.3f" % en[(r + 1) * len(groups)] for r in range(3)]))


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
TIE_CASES = [lambda: C.tree_model(C.TREE7, (6,) * 7, "dense", seed=16, ints=True), lambda: C.tree_model(C.TREE7, (6,) * 7, "potts", seed=17, ints=True),
             lambda: C.tree_model(C.TREE7, (6,) * 7, "diff", seed=18, ints=True), lambda: C.fan_case(8)]


def test_the_tie_cases_tell_the_first_minimiser_from_the_last():
    """quantised costs with zero messages: ties everywhere.  The rule takes the SMALLEST minimiser in the back-pointers and at the
    roots; a "largest minimiser" variant reaches the same energy (both are minimisers) with other labels on at least one of the
    quantised cases, so the tie cases of the GPU tests have teeth.  On the continuous case (no ties) the variant changes nothing."""
    differ = []
    for make in TIE_CASES[:3]:
        m, groups = make()
        start = C.random_primal(m, 7)
        a = C.forest_moves_reference(m, m.dual_data, start, groups[:1])
        b = C.forest_moves_reference(m, m.dual_data, start, groups[:1], variant="last")
        assert abs(C.energy(m, a) - C.energy(m, b)) <= 1e-12
        differ.append(not np.array_equal(a, b))
    assert any(differ), differ
    m, groups = TIE_CASES[3]()
    start = C.random_primal(m, 7)
    assert np.array_equal(C.forest_moves_reference(m, m.dual_data, start, groups), C.forest_moves_reference(m, m.dual_data, start, groups, variant="last"))


# ---- lpmp_plan_forest_info: counts ---------------------------------------------------------------------------------------------------
def test_counts_on_hand_counted_cases():
    m, groups = C.tree_model()            # TREE7 and an off-tree neighbour each
    p = E.Plan(m)
    assert p.forest_info(groups) == {"n_trees": 1 + 7, "n_tree_edges": 6, "n_off_tree_links": 7 + 7, "max_height": 2}
    assert p.forest_info(groups[:1]) == {"n_trees": 1, "n_tree_edges": 6, "n_off_tree_links": 7, "max_height": 2}
    assert p.forest_info(groups[1:]) == {"n_trees": 7, "n_tree_edges": 0, "n_off_tree_links": 7, "max_height": 0}
    assert p.forest_info([]) == p.forest_info([([], []), ([], [])]) == {"n_trees": 0, "n_tree_edges": 0, "n_off_tree_links": 0, "max_height": 0}
    # the same unary in two groups, a sub-forest of two trees: {1 <- 3, 4} and {2 <- 6}
    assert p.forest_info([([1, 3, 4, 2, 6], [-1, 1, 1, -1, 2]), ([0], [-1])]) == {"n_trees": 3, "n_tree_edges": 3, "n_off_tree_links": (5 + 3) + (1 + 2), "max_height": 1}
    # a chain rooted at its end: the height is its length in edges
    m, pg = PC.ladder((3, 3, 3, 3, 3), "dense", seed=2)
    assert E.Plan(m).forest_info(M.forests_from_paths(pg)) == {"n_trees": 2, "n_tree_edges": 8, "n_off_tree_links": 10, "max_height": 4}
    # the star rooted at the hub and at a leaf
    m = DC.star()
    leaves = [v for v in range(71) if v != 35]
    assert E.Plan(m).forest_info([([35] + leaves, [-1] + [35] * 70)]) == {"n_trees": 1, "n_tree_edges": 70, "n_off_tree_links": 0, "max_height": 1}
    assert E.Plan(m).forest_info([([35] + leaves, [0] + [-1] + [35] * 69)]) == {"n_trees": 1, "n_tree_edges": 70, "n_off_tree_links": 0, "max_height": 2}


# ---- refusals, in their order ----------------------------------------------------------------------------------------------------------
def _refusal(m, groups, code):
    with pytest.raises(E.EngineError) as ei:
        E.Plan(m).forest_info(groups)
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


def _raw_info(m, group_off, unaries, parent):
    p = E.Plan(m)
    go, un, par = np.asarray(group_off, np.int64), np.asarray(unaries + [0], np.int32), np.asarray(parent + [0], np.int32)
    buf = ctypes.create_string_buffer(512)
    rc = p.L.lpmp_plan_forest_info(p.h, go.shape[0] - 1, go.ctypes.data, un.ctypes.data, par.ctypes.data, None, None, None, None, buf, 512)
    return rc, buf.value.decode()


def test_invalid_sets_name_the_entry():
    H, W = 4, 5
    m = PC.grid(H, W, 3, "row_major")           # unary of (r, c): r * W + c; pairwise factors from H * W on
    # offsets
    rc, why = _raw_info(m, [0, 2, 1], [0, 2], [-1, -1])
    assert rc == ERR_INVALID and "group_off" in why and "group 1" in why
    rc, why = _raw_info(m, [1, 2], [0, 2], [-1, -1])
    assert rc == ERR_INVALID and "group_off[0]" in why
    rc, why = _raw_info(m, [0, 1], [0], [-1])
    assert rc == 0 and why == ""
    # indices and kinds (before anything about parents: entry 0 has a bad parent too)
    why = _refusal(m, [([0, 1, H * W + 100000], [7, 0, 1])], ERR_INVALID)
    assert "out of range" in why and "entry 2" in why
    why = _refusal(m, [([0, -1], [-1, 0])], ERR_INVALID)
    assert "out of range" in why and "entry 1" in why
    why = _refusal(m, [([0, 1], [-1, 0]), ([H * W], [-1])], ERR_INVALID)
    assert "factor %d " % (H * W) in why and "entry 2" in why and "not a VECTOR" in why
    # a unary twice in one group (before the parents: entry 1 is its own parent); in two GROUPS it is fine
    why = _refusal(m, [([0, 1, 0], [-1, 1, 1])], ERR_INVALID)
    assert "factor 0 " in why and "entry 2" in why and "twice in group 0" in why and "entry 0" in why
    assert E.Plan(m).forest_info([([0, 1], [1, -1]), ([0, 1], [-1, 0])])["n_trees"] == 2
    # parents: itself, not a member, a member of another group only, out of range
    why = _refusal(m, [([0, 1], [-1, 1])], ERR_INVALID)
    assert "factor 1 (entry 1)" in why and "its own parent" in why
    why = _refusal(m, [([0, 1], [-1, 2])], ERR_INVALID)
    assert "parent 2 of factor 1 (entry 1)" in why and "member of group 0" in why
    why = _refusal(m, [([2], [-1]), ([0, 1], [-1, 2])], ERR_INVALID)
    assert "parent 2 of factor 1 (entry 2)" in why and "member of group 1" in why
    why = _refusal(m, [([0, 1], [-2, 0])], ERR_INVALID)
    assert "parent -2 of factor 0 (entry 0)" in why
    why = _refusal(m, [([0, 1], [-1, H * W])], ERR_INVALID)
    assert "parent %d of factor 1 (entry 1)" % (H * W) in why
    # cycles of parent pointers: the lowest entry on one; the tail that leads into it is not named (before the missing edge 3 - 0)
    why = _refusal(m, [([7], [-1]), ([4, 3, 2, 1, 0], [3, 2, 1, 3, -1])], ERR_INVALID)
    assert "cycle" in why and "factor 3 (entry 2)" in why
    why = _refusal(m, [([0, 1], [1, 0])], ERR_INVALID)
    assert "cycle" in why and "factor 0 (entry 0)" in why
    # a child and its parent joined by no pairwise factor
    why = _refusal(m, [([0, 1, W + 2], [-1, 0, 1])], ERR_INVALID)
    assert "no pairwise factor joins" in why and "factor %d (entry 2)" % (W + 2) in why and "factor 1 (entry 1)" in why
    # a chord: the four unaries of a grid cell as a chain 0 <- 1 <- W + 1 <- W; and an edge between two trees
    why = _refusal(m, [([0, 1, W + 1, W], [-1, 0, 1, W + 1])], ERR_INVALID)
    assert "not child and parent" in why and "induce a forest" in why and "factor 0 (entry 0)" in why and "factor %d (entry 3)" % W in why
    why = _refusal(m, [([0, 1, W, W + 1], [-1, 0, -1, W])], ERR_INVALID)
    assert "not child and parent" in why and "factor 0 (entry 0)" in why and "factor %d (entry 2)" % W in why
    # the parallel edges of duplicate_edges: variables 0 and 1 are joined by three pairwise factors
    why = _refusal(DC.duplicate_edges(), [([2, 1, 0], [1, 0, -1])], ERR_INVALID)
    assert "more than one pairwise factor" in why and "factor 1 (entry 1)" in why and "factor 0 (entry 2)" in why
    assert E.Plan(DC.duplicate_edges()).forest_info([([2, 1], [1, -1]), ([0], [-1])])["n_tree_edges"] == 1


def test_unsupported_sets_name_the_lowest_listed_unary_and_come_after_the_invalid_ones_of_the_first_kind():
    mc = S.multicut_triangle_model(6, 4, seed=1)
    why = _refusal(mc, [([3, 1], [-1, -1]), ([2], [-1])], ERR_UNSUPPORTED)
    assert "factor 1 " in why and "not a unary-pairwise message" in why and "forest moves" in why
    why = _refusal(mc, [([3, 1], [1, 3])], ERR_INVALID)            # a cycle is reported first
    assert "cycle" in why
    m5 = S.c5_model(5, 4, 4, 12, 6, 3, seed=2, window=12)
    assert E.Plan(m5).forest_info(M.forests_from_paths(S.grid_paths(5, 4, "colour_major")))["n_trees"] == 9
    r = np.random.default_rng(0)
    un = [r.random(3) for _ in range(4)]
    T = lambda: ("dense", r.random((3, 3)))
    edges = [(0, 1, T()), (1, 2, T()), (2, 3, T())]          # pairwise factors 4, 5, 6
    both = [(0, 0, 0), (1, 1, 0), (0, 1, 1), (1, 2, 1), (0, 2, 2), (1, 3, 2)]
    assert E.Plan(C.build_model(un, edges, both)).forest_info([([0, 1, 2, 3], [1, 2, 3, -1])])["n_tree_edges"] == 3
    # factor 5 has no unary on side 1: unary 1 is the lowest listed one next to it — reported before the missing tree edge 1 - 3
    lame = C.build_model(un, edges, [x for x in both if x != (1, 2, 1)])
    why = _refusal(lame, [([3, 1], [-1, 3]), ([0], [-1])], ERR_UNSUPPORTED)
    assert "factor 1 " in why and "pairwise factor 5" in why and "exactly one unary on each side" in why
    assert E.Plan(lame).forest_info([([3, 0], [-1, -1])])["n_trees"] == 2
    # more than 512 labels
    big = C.build_model([r.random(513), r.random(2), r.random(512)], [(0, 1, ("dense", r.random((513, 2)))), (2, 1, ("dense", r.random((512, 2))))])
    why = _refusal(big, [([2, 1, 0], [1, -1, 1])], ERR_UNSUPPORTED)
    assert "factor 0 " in why and "513 labels" in why
    assert E.Plan(big).forest_info([([2, 1], [1, -1])])["n_tree_edges"] == 1


# ---- the suggested cover -------------------------------------------------------------------------------------------------------------
def _check_cover(m, groups):
    """every group is accepted, alone and together; every tree is rooted at a centre.  Returns the unaries covered"""
    p = E.Plan(m)
    info = p.forest_info(groups)
    covered = set()
    heights = []
    for un, par in groups:
        assert un.dtype == np.int32 and par.dtype == np.int32 and len(set(un.tolist())) == len(un)
        assert p.forest_info([(un, par)])["n_trees"] == int(np.sum(par == -1))
        covered |= set(un.tolist())
        h, d = C.tree_stats(un, par)
        assert h == [(x + 1) // 2 for x in d], (h, d)              # rooted at a centre: height = ceil(diameter / 2)
        heights += h
    assert info["max_height"] == max(heights, default=0)
    return covered


@pytest.mark.parametrize("name", ["random_graph", "thinned_grid", "star", "grid_row", "grid_colour", "mixed", "duplicate"])
def test_suggested_cover(name):
    m = {"random_graph": DC.random_graph, "thinned_grid": C.thinned_grid, "star": DC.star, "grid_row": lambda: PC.grid(12, 9, 5, "row_major"),
         "grid_colour": lambda: PC.grid(12, 9, 5, "colour_major"), "mixed": DC.mixed_case, "duplicate": DC.duplicate_edges}[name]()
    p = E.Plan(m)
    left = []
    groups = p.suggest_forests(left_out=left)
    unaries, _ = C.structure(m)
    assert left == [0]
    assert _check_cover(m, groups) == set(unaries)          # every eligible unary is in at least one group
    assert 1 <= len(groups) <= C.graph_degree(m) // 2 + 1
    # deterministic, twice over
    for _ in range(2):
        again = E.Plan(m).suggest_forests()
        assert len(again) == len(groups) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(again, groups))
    # max_groups truncates
    for k in range(1, len(groups) + 1):
        part = p.suggest_forests(max_groups=k)
        assert len(part) == k and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(part, groups))
    # the first group is maximal: every unary outside it has two links into one of its trees, so it would close a cycle
    first = set(groups[0][0].tolist())
    _, links = C.structure(m)
    for u in sorted(set(unaries) - first):
        assert len([w for _, _, w in links[u] if w in first]) >= 2
        with pytest.raises(E.EngineError) as ei:
            p.forest_info([(np.append(groups[0][0], u).astype(np.int32), np.append(groups[0][1], -1).astype(np.int32))])
        assert ei.value.code == ERR_INVALID and "induce a forest" in str(ei.value)


def test_suggested_cover_of_tree_models_is_one_tree():
    for s in range(6):
        m, parents = C.random_tree(s)
        groups = E.Plan(m).suggest_forests()
        assert len(groups) == 1 and int(np.sum(groups[0][1] == -1)) == 1 and sorted(groups[0][0].tolist()) == list(range(len(parents)))
        _check_cover(m, groups)
        best = C.brute_force(m)
        pr = C.forest_moves_reference(m, m.dual_data, C.random_primal(m, s), groups)
        assert abs(C.energy(m, pr) - best) <= 1e-12 * max(1.0, abs(best))
    m, pg = PC.long_case()                   # two rails of 300 joined by rungs: the first group holds a spanning comb or similar
    groups = E.Plan(m).suggest_forests()
    _check_cover(m, groups)
    assert len(groups) <= 2


def test_suggested_cover_leaves_exactly_the_ineligible_unaries_out():
    """the Potts grid of c5_model with labeling-list factors beside it: the unaries that carry a labeling message are left out"""
    H, W = 5, 4
    m5 = S.c5_model(H, W, 4, 12, 6, 3, seed=2, window=12)
    p = E.Plan(m5)
    bad = {int(m5.m_left[k]) for k in range(m5.n_messages) if m5.mtypes[int(m5.m_type[k])].kind != M.M_UNARY_PAIRWISE} | \
          {int(m5.m_right[k]) for k in range(m5.n_messages) if m5.mtypes[int(m5.m_type[k])].kind != M.M_UNARY_PAIRWISE}
    vec = {f for f in range(m5.n_factors) if m5.f_kind[f] == M.F_VECTOR}
    left = []
    groups = p.suggest_forests(left_out=left)
    covered = set()
    for un, par in groups:
        covered |= set(un.tolist())
    assert left == [len(vec & bad)] and left[0] > 0
    assert covered == vec - bad and set(range(H * W)) <= covered
    p.forest_info(groups)
    # a model nothing of which is eligible: no group
    mc = S.multicut_triangle_model(6, 4, seed=1)
    left = []
    assert E.Plan(mc).suggest_forests(left_out=left) == [] and left[0] == sum(1 for f in range(mc.n_factors) if mc.f_kind[f] == M.F_VECTOR)


def test_forests_from_paths():
    g = M.forests_from_paths([[[3, 4, 5], [9]], [], [[7, 6]]])
    assert [(u.tolist(), q.tolist()) for u, q in g] == [([3, 4, 5, 9], [4, 5, -1, -1]), ([], []), ([7, 6], [6, -1])]
    assert all(u.dtype == np.int32 and q.dtype == np.int32 for u, q in g)


def test_abi_declares_and_exports_the_calls():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "lpmp_engine.h")).read()
    L = E.lib()
    assert "typedef struct lpmp_forest_set lpmp_forest_set;" in hdr
    for fn in NEW_INT:
        assert re.search(r"\bint %s\(" % fn, hdr) and fn in E.EXPORTS and hasattr(L, fn)
    assert re.search(r"\bvoid lpmp_forest_set_destroy\(", hdr)
    for fn in NEW_OTHER[1:]:
        assert re.search(r"\bint64_t %s\(const lpmp_forest_set\*" % fn, hdr)
    for fn in NEW_OTHER:
        assert fn in E.EXPORTS and hasattr(L, fn)
