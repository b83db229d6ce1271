"""Conditional rounding from the duals, host side: the planner's decode levels against the numpy recurrence, the
refusals, the numpy statement of the rule (tests/decode_cases.py) against brute force and against itself over refinement sweeps
on duals of the CPU oracle, and the ABI.  No GPU."""
import os
import re

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import decode_cases as C

ANISO = M.REPAM_ANISOTROPIC
ERR_UNSUPPORTED = -2
NEW = ("lpmp_decode_primal", "lpmp_plan_decode_info", "lpmp_plan_get_decode_levels")

LEVEL_MODELS = {
    "grid_row_major": lambda: C.grid(7, 6, 4, "row_major"),
    "grid_colour_major": lambda: C.grid(7, 6, 4, "colour_major"),
    "random_graph": lambda: C.random_graph(),
    "star70": lambda: C.star(),
    "duplicate_edges": lambda: C.duplicate_edges(),
    "mixed": lambda: C.mixed_case(),
}


@pytest.mark.parametrize("name", sorted(LEVEL_MODELS))
def test_decode_levels_equal_the_recurrence(name):
    m = LEVEL_MODELS[name]()
    p = E.Plan(m)
    for d in (0, 1):
        f, lv = p.decode_levels(d)
        rf, rlv = C.level_reference(m, p.order(d))
        assert np.array_equal(f, rf) and np.array_equal(lv, rlv), (name, d)
        info = p.decode_info(d)
        assert info == {"n_unaries": int((m.f_kind == M.F_VECTOR).sum()), "n_levels": int(rlv.max()), "n_links": m.n_messages}
        # neighbours never share a level, and the later one in the order has the higher level
        level = dict(zip(f.tolist(), lv.tolist()))
        pos = {u: i for i, u in enumerate(f.tolist())}
        for u, links in C.structure(m)[1].items():
            for _, _, v in links:
                assert (level[u] < level[v]) == (pos[u] < pos[v]) and level[u] != level[v]
    if name == "grid_row_major":
        assert [p.decode_info(d)["n_levels"] for d in (0, 1)] == [12, 12]
    if name == "grid_colour_major":
        assert [p.decode_info(d)["n_levels"] for d in (0, 1)] == [2, 2]
    if name == "star70":
        assert [p.decode_info(d)["n_levels"] for d in (0, 1)] == [3, 3]


def _refused(m):
    p = E.Plan(m)
    out = []
    for d in (0, 1):
        for call in (lambda: p.decode_info(d), lambda: p.decode_levels(d)):
            with pytest.raises(E.EngineError) as ei:
                call()
            assert ei.value.code == ERR_UNSUPPORTED
            out.append(str(ei.value))
    assert len(set(out)) == 1
    return out[0]


def test_refusals_name_the_lowest_offending_factor():
    r = np.random.default_rng(0)
    L = 3
    un = [r.random(L) for _ in range(4)]
    T = lambda: ("dense", r.random((L, L)))
    # factors: unaries 0 .. 3, pairwise 4, 5, 6
    edges = [(0, 1, T()), (1, 2, T()), (2, 3, T())]
    both = [(0, 0, 0), (1, 1, 0), (0, 1, 1), (1, 2, 1), (0, 2, 2), (1, 3, 2)]
    assert E.Plan(C.build_model(un, edges, both)).decode_info(0)["n_levels"] == 4
    # factor 5 has no unary on side 1; factor 6 none on side 0: the lower one is named
    why = _refused(C.build_model(un, edges, [x for x in both if x not in ((1, 2, 1), (0, 2, 2))]))
    assert "factor 5 " in why and "no unary" in why
    # two unaries on side 0 of factor 6
    why = _refused(C.build_model(un, edges, both + [(0, 0, 2)]))
    assert "factor 6 " in why and "two unaries" in why
    # unary 1 on both sides of factor 4
    why = _refused(C.build_model(un, edges, [(0, 1, 0), (1, 1, 0)] + both[2:]))
    assert "factor 4 " in why and "both sides" in why
    # a pairwise factor without any message
    why = _refused(C.build_model(un, edges, both[:4]))
    assert "factor 6 " in why and "no unary" in why
    # another message kind: the lowest factor of such a message
    m = S.multicut_triangle_model(6, 4, seed=1)
    bad = min(min(int(m.m_left[k]), int(m.m_right[k])) for k in range(m.n_messages) if m.mtypes[int(m.m_type[k])].kind != M.M_UNARY_PAIRWISE)
    why = _refused(m)
    assert ("factor %d " % bad) in why and "not a unary-pairwise" in why


def test_chains_decode_to_the_optimum_against_the_last_sweep():
    """20 random chains (6 variables, 3 labels): after ComputePass(2), which ends with a backward sweep, the FORWARD decode is the
    brute-force optimum on every chain; after one more forward sweep the BACKWARD decode is.  The other direction is not: the
    counts are printed (DESIGN.md 8 quotes them)."""
    hits = {"fwd_after_bwd": 0, "bwd_after_bwd": 0, "bwd_after_fwd": 0, "fwd_after_fwd": 0}
    for seed in range(20):
        m = C.chain(seed)
        best = C.brute_force(m)
        o = Oracle(m)
        o.set_reparametrization(ANISO)
        o.ComputePass(2)
        e = [C.energy(m, C.decode_reference(m, o.duals(), o.order(d))) for d in (0, 1)]
        o.ComputeForwardPass()
        e2 = [C.energy(m, C.decode_reference(m, o.duals(), o.order(d))) for d in (0, 1)]
        tol = 1e-12 * max(1.0, abs(best))
        assert abs(e[0] - best) <= tol, (seed, e, best)
        assert abs(e2[1] - best) <= tol, (seed, e2, best)
        hits["fwd_after_bwd"] += abs(e[0] - best) <= tol
        hits["bwd_after_bwd"] += abs(e[1] - best) <= tol
        hits["bwd_after_fwd"] += abs(e2[1] - best) <= tol
        hits["fwd_after_fwd"] += abs(e2[0] - best) <= tol
    print("chains decoded to the optimum, of 20:", hits)
    assert hits["fwd_after_bwd"] == 20 and hits["bwd_after_fwd"] == 20


@pytest.mark.parametrize("kind", ["random", "truncated"])
@pytest.mark.parametrize("order", ["row_major", "colour_major"])
def test_energy_does_not_rise_over_refinement_sweeps(kind, order):
    """a refinement sweep is ICM on the original energy.  Slack 1e-9 * max(1, |E|): the energies are sums of ~1700 terms of
    magnitude <= 1, whose rounding error is below 1e-15 * 1700 * |E| — six orders under the slack"""
    m = C.table_grid(kind, order)
    o = Oracle(m)
    o.set_reparametrization(ANISO)
    done = 0
    for passes in (5, 50):
        o.ComputePass(passes - done)
        done = passes
        sweeps = []
        C.decode_reference(m, o.duals(), o.order(0), refine=3, sweeps_out=sweeps)
        en = [C.energy(m, s) for s in sweeps]
        print(kind, order, passes, "passes: bound", o.LowerBound(), "decode and 3 refinement sweeps", en)
        assert len(en) == 4
        for a, b in zip(en, en[1:]):
            assert b <= a + 1e-9 * max(1.0, abs(a))
        assert en[-1] >= o.LowerBound() - 1e-9 * max(1.0, abs(en[-1]))


def test_abi_declares_and_exports_the_calls():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "lpmp_engine.h")).read()
    L = E.lib()
    for fn in NEW:
        assert re.search(r"\bint %s\(" % fn, hdr) and fn in E.EXPORTS and hasattr(L, fn)
    for hxx in ("LP_gpu.hxx", "lpmp_offload.hxx"):
        src = open(os.path.join(os.path.dirname(__file__), "..", "lp_mp_amd", "include", hxx)).read()
        assert "lpmp_decode_primal(engine_" in src
