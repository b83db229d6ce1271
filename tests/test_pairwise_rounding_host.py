"""Pairwise factors that round themselves, on the host (tests/pairwise_rounding_cases.py has the case list and the numpy
statement of the rule): the rule pinned against the oracle's hooks, proof that the list tells wrong rules apart, the expansion
against the kind, the census of kernel classes the list reaches, and what the planner promises about such records.  No GPU
needed."""
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pairwise_rounding_cases as PR              # noqa: E402
import schedule_hazards as H                      # noqa: E402
from lp_mp_amd import engine as E                 # noqa: E402
from lp_mp_amd import model as M                  # noqa: E402
from oracle.binding import Oracle                 # noqa: E402

WRONG = ("last", "column_major", "ignore_given")


@pytest.fixture(scope="module")
def probe_lib(tmp_path_factory):
    return H.build_probe(tmp_path_factory.mktemp("schedule_probe"))


def _close(c, co):
    return (c == co) if np.isinf(co) else abs(c - co) <= 1e-9 * max(1.0, abs(co))       # test_primal_gpu._same


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule against the oracle's hooks

def _small_models():
    """(name, case) of 1 - 3-factor models of every kind: one pairwise factor with two unaries, a 3-chain, and the 3-chain with two
    more factors that have a unary on one side only"""
    for kind in PR.KINDS:
        d0, d1 = (5, 5) if kind == "potts" else (5, 7)
        for struct in (("chain", 1), ("chain", 3), ("one_sided",)):
            for sched, computes in PR.COMBOS:
                for values in ("u01", "quant"):
                    yield PR.Case(kind, d0, d1, struct, sched, computes, values=values, seed=70)


def _presets(m, rng):
    """labellings for every combination of given sides: no unary labelled, the even ones (side 0 of the first factor), the odd
    ones (its side 1), all; with a one-sided factor also its own slot on the side without a unary"""
    n = int(np.sum(m.f_kind == M.F_VECTOR))
    side_unary, _ = PR.links(m)
    even = [k % 2 == 0 for k in range(n)]
    for name, on in (("none", [False] * n), ("side 0", even), ("side 1", [not x for x in even]), ("both", [True] * n)):
        pr = PR.consistent_preset(m, on, rng)
        yield name, pr
        own = [(p, s) for p in range(n, m.n_factors) for s in (0, 1) if (p, s) not in side_unary]
        if own:
            pr = pr.copy()
            for p, s in own:
                pr[p, s] = int(rng.integers(0, (m.f_dim0 if s == 0 else m.f_dim1)[p]))
            yield name + ", own slots", pr


def test_the_numpy_rule_is_the_oracles_hook_on_small_models_of_every_kind():
    """one rounding sweep of the oracle (on the expansion) against the numpy rule (on the kind), forward and backward, from the
    duals after one plain pass, for every combination of given sides preset through Oracle.set_primal at the stamp of the
    sweep"""
    rng = np.random.default_rng(11)
    checked = Counter()
    for c in _small_models():
        m, y = c.model, c.yardstick
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            o = Oracle(y)
            o.set_reparametrization(mode)
            o.ComputePass(1)
            duals0 = o.duals()
            for pname, pr in _presets(m, rng):
                for d, stamp in ((M.FORWARD, 1), (M.BACKWARD, 2)):
                    o.set_duals(duals0)
                    o.set_primal(pr, stamp)
                    (o.ComputeForwardPassAndPrimal if d == M.FORWARD else o.ComputeBackwardPassAndPrimal)(0)
                    want = PR.simulate_sweep(m, y, d, mode, duals0, pr)
                    assert np.array_equal(o.primal(), want), (c.name, mode, pname, d)
                    checked[(c.kind, pname.split(",")[0])] += 1
    for kind in PR.KINDS:
        for pname in ("none", "side 0", "side 1", "both"):
            assert checked[(kind, pname)] > 0, (kind, pname)


def _shift_2x3():
    """one 2 x 3 DIFF_SHIFT factor whose index clamps at both ends: D = [1, 4], scale 0.5, shift 1, index clip(a - b + 1, 0, 1):
        cost = [[2.0, 0.5, 0.5],       (a = 0: indices 1, 0, -1 -> 0)
                [2.0, 2.0, 0.5]]       (a = 1: indices 2 -> 1, 1, 0)
    with m1 = [0.25, 0], m2 = [0, 0.25, 0.5]:  cost + m1 + m2 = [[2.25, 1.0, 1.25], [2.0, 2.25, 1.0]]"""
    D = np.array([1.0, 4.0])
    # (`right` schedule, only the pairwise type rounds: the factor is the one update of a sweep, and what it receives is +0.0)
    m = PR.build([np.zeros(2), np.zeros(3)], [(0, 1, ("shift", D, 0.5, 1, (2, 3)))], M.SCHED_RIGHT, (0, 1))
    duals = np.concatenate([np.zeros(5), [0.25, 0.0], [0.0, 0.25, 0.5]])
    return m, duals


def test_hand_computed_values_of_a_clamping_diff_shift_factor():
    m, duals = _shift_2x3()
    y = PR.oracle_model(m)
    assert np.array_equal(y.const_data, [2.0, 0.5, 0.5, 2.0, 2.0, 0.5])
    # given sides -> labels: nothing given: the minimum 1.0 is at (0, 1) and (1, 2), the first in row-major order is (0, 1)
    want = {(None, None): (0, 1), (1, None): (1, 2), (0, None): (0, 1), (None, 0): (1, 0), (None, 2): (1, 2),
            (0, 2): (0, 2), (1, 0): (1, 0)}
    doff, coff = m.dual_offsets(), m.const_offsets()
    side_unary, _ = PR.links(m)
    for (g0, g1), (x0, x1) in want.items():
        pr = PR.unset_primal(m)
        if g0 is not None:
            pr[0, 0] = pr[2, 0] = g0
        if g1 is not None:
            pr[1, 0] = pr[2, 1] = g1
        assert PR.round_pairwise(m, coff, doff, duals, pr, 2, side_unary)[:2] == (x0, x1), (g0, g1)
        o = Oracle(y)
        o.set_reparametrization(M.REPAM_ANISOTROPIC)
        o.set_duals(duals)
        o.set_primal(pr, 1)
        o.ComputeForwardPassAndPrimal(0)
        got = o.primal()
        assert (got[2, 0], got[2, 1]) == (x0, x1) and (got[0, 0], got[1, 0]) == (x0, x1), (g0, g1, got)
    # the seeded wrong rules on the same numbers
    pr = PR.unset_primal(m)
    assert PR.round_pairwise(m, coff, doff, duals, pr, 2, side_unary, "last")[:2] == (1, 2)
    assert PR.round_pairwise(m, coff, doff, duals, pr, 2, side_unary, "column_major")[:2] == (0, 1)
    pr[0, 0] = pr[2, 0] = 1
    assert PR.round_pairwise(m, coff, doff, duals, pr, 2, side_unary, "ignore_given")[:2] == (0, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the list discriminates

def test_quantised_and_zero_cases_tell_three_wrong_rules_apart_on_every_kind():
    """on the quantised and all-zero cases the numpy rule reproduces the oracle's first rounding sweeps (forward from the original
    costs, backward from the duals after it), and each seeded wrong rule — the last minimiser, column-major tie order, ignoring
    the given side — gives other labels than the oracle on at least one case of every kind"""
    told = Counter()
    for c in PR.CASES:
        if c.values not in ("quant", "zero"):
            continue
        m, y = c.model, c.yardstick
        o = Oracle(y)
        o.set_reparametrization(M.REPAM_ANISOTROPIC)
        duals0 = o.duals()
        unset = PR.unset_primal(m)
        assert np.array_equal(o.primal(), unset), c.name
        o.ComputeForwardPassAndPrimal(0)
        fwd, duals1 = o.primal(), o.duals()
        o.ComputeBackwardPassAndPrimal(0)
        bwd = o.primal()
        for d, d0, want in ((M.FORWARD, duals0, fwd), (M.BACKWARD, duals1, bwd)):
            assert np.array_equal(PR.simulate_sweep(m, y, d, M.REPAM_ANISOTROPIC, d0, unset), want), (c.name, d)
            if max(c.d0, c.d1) > 8 and d == M.BACKWARD:
                continue                              # (the wrong rules: the forward sweep of the larger cases is enough)
            for v in WRONG:
                if not np.array_equal(PR.simulate_sweep(m, y, d, M.REPAM_ANISOTROPIC, d0, unset, variant=v), want):
                    told[(c.kind, v)] += 1
    print("\ncases that tell a wrong rule apart:", dict(told))
    missing = [(kind, v) for kind in PR.KINDS for v in WRONG if told[(kind, v)] == 0]
    assert not missing, "no quantised or all-zero case separates (kind, wrong rule): %r" % (missing,)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. expansion equals kind

@pytest.mark.parametrize("kind", PR.KINDS)
def test_energy_on_the_kind_equals_the_cost_of_the_expansion(kind):
    """every case: the loop of the GPU test on the oracle alone — every rounding sweep ends consistent, with a finite cost that
    is the numpy energy of the labels on the kind model's original costs, and the best cost is no less than the bound"""
    n = 0
    for c in PR.CASES:
        if c.kind != kind:
            continue
        m = c.model
        o = Oracle(c.yardstick)
        o.set_reparametrization(PR.MODES[n % 4])
        best = np.inf
        for it in range(2):
            for sweep in (o.ComputeForwardPassAndPrimal, o.ComputeBackwardPassAndPrimal):
                sweep(it)
                assert o.CheckPrimalConsistency(), c.name
                cost = o.EvaluatePrimal()
                assert np.isfinite(cost), c.name
                assert _close(PR.energy(m, o.primal()), cost), (c.name, PR.energy(m, o.primal()), cost)
                best = min(best, cost)
            o.ComputePass(1)
        lb = o.LowerBound()
        assert best >= lb - 1e-9 * max(1.0, abs(lb)), (c.name, best, lb)
        n += 1
    assert n > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 4. census

# pairwise4 is not in the list: a factor of at most 4 labels a side has d0 + d1 <= 8 and every op of it at most 4 entries, so
# plan.cpp (cls_of: small_ok before the packed classes) gives it the lane-per-factor class whatever its messages are — no model
# reaches pairwise4 through the planner.  The census asserts that too: should the planner ever hand the class out, it fails here.
PAIRWISE_CELLS = ("small", "pairwise8", "pairwise16", "pairwise32", "generic")
PACKED_DENSE = {"dense4", "dense8", "dense16", "dense32", "dense_v4", "dense_v8", "dense_v16", "dense_v32"}
PACKED_POTTS = {"potts4", "potts8", "potts16", "potts32", "potts_v4", "potts_v8", "potts_v16", "potts_v32"}
SHARED = {"shared4", "shared8", "shared16", "shared32"}


def _expected_pairwise_cell(kind, d0, d1):
    """plan.cpp cls_of: lane per factor up to d0 + d1 = 8; the packed pairwise classes hold DENSE and POTTS factors of at most 32
    labels (those launches are rerouted in primal passes); the pooled kinds and everything larger run the generic kernel always"""
    w = max(d0, d1)
    if d0 + d1 <= 8:
        return "small"
    if w > 32 or kind not in (M.F_PAIRWISE_DENSE, M.F_PAIRWISE_POTTS):
        return "generic"
    return "pairwise%d" % (4 if w <= 4 else 8 if w <= 8 else 16 if w <= 16 else 32)


def test_census_every_cell_is_reached_and_nothing_is_skipped(probe_lib):
    """the classes of every case, per record.  The updated pairwise factors take the class their kind and label counts name: lane
    per factor up to d0 + d1 = 8; pairwise8 ... 32 for DENSE and POTTS factors; generic above 32 labels and for the pooled kinds,
    with or without an active message in the sweep (the packed kernel reads a d0 x d1 table, which a pooled factor does not
    hold).  The list as a whole reaches every pairwise cell and — where the unaries round too — every unary class that calls
    store_label: diff (plain, banded, shifted), shared*, dense_big, packed dense and packed Potts.  A case the planner refuses
    raises here: nothing is skipped."""
    pw_cells, unary_cells, by_kind = Counter(), Counter(), {}
    for c in PR.CASES:
        classes, pairwise, unary = PR.census(c, probe_lib)
        m = c.model
        pw = np.flatnonzero(m.f_kind != M.F_VECTOR)
        want = {_expected_pairwise_cell(int(m.f_kind[p]), int(m.f_dim0[p]), int(m.f_dim1[p])) for p in pw}
        assert pairwise == want, (c.name, pairwise, want)
        assert all(int(m.f_dim0[p]) + int(m.f_dim1[p]) <= 512 for p in pw), c.name
        for cell in pairwise:
            pw_cells[cell] += 1
        if c.computes == (1, 1):
            assert unary, c.name
            for cell in unary:
                unary_cells[cell] += 1
            by_kind.setdefault(c.kind, set()).update(unary)
        else:
            assert not unary or c.sched == "full", (c.name, unary)     # `right`: a unary that does not round is not updated at all
    print("\npairwise records:", dict(pw_cells), "\nunary records where the unaries round:", dict(unary_cells))
    for cell in PAIRWISE_CELLS:
        assert pw_cells[cell] > 0, cell
    assert set(pw_cells) == set(PAIRWISE_CELLS), dict(pw_cells)           # (no pairwise4, see above; nothing unexpected)
    for cell in ("diff", "diff:plain", "diff:banded", "diff:shifted", "dense_big"):
        assert unary_cells[cell] > 0, cell
    for name, group in (("shared*", SHARED), ("packed dense", PACKED_DENSE), ("packed Potts", PACKED_POTTS)):
        assert any(unary_cells[x] > 0 for x in group), name
    assert "diff:banded" in by_kind["diff_band"] and "diff:shifted" in by_kind["diff_shift"] and by_kind["shared"] & SHARED
    # d0 + d1 = GEN_MAXD is reached, twice
    sizes = Counter(c.d0 + c.d1 for c in PR.CASES)
    assert sizes[512] >= 2 and max(sizes) == 512


def test_every_grid_of_at_most_40_labels_comes_in_both_variable_orders():
    """row-major grids make deep schedules (level loops / chains in the plain passes), colour-major ones wide levels: every kind
    has both at every label count up to 40, with u01 costs"""
    orders = {}
    for c in PR.CASES:
        if c.struct[0] == "grid" and c.d0 <= 40 and c.values == "u01":
            orders.setdefault((c.kind, c.d0), set()).add(c.struct[3])
    squares = [s[0] for s in PR.SMALL + PR.PACKED + PR.GENERIC if s[0] == s[1] and s[0] <= 40]
    for kind in PR.KINDS:
        if kind != "mixed":                                   # (the mixed model is a hub, not a grid)
            for L in squares:
                assert orders.get((kind, L)) == set(PR.ORDERS), (kind, L, orders.get((kind, L)))


def test_every_kind_with_table_or_vector_entries_has_cases_with_holes():
    """+inf entries: every kind but Potts (a scalar) and the banded DIFF vectors (truncated linear: no entry to take out)"""
    have = {c.kind for c in PR.CASES if c.values == "inf"}
    assert have == set(PR.KINDS) - {"potts", "diff_band"}, have
    for c in PR.CASES:
        if c.values == "inf":
            assert np.isinf(c.yardstick.const_data).any(), c.name


def test_banded_cases_are_banded_by_the_planner():
    for c in PR.CASES:
        if c.kind == "diff_band":
            bands = E.Plan(c.model).diff_bands()
            assert bands and all(b[2] for b in bands.values()), (c.name, bands)
        elif c.kind == "diff" and c.values == "u01":
            bands = E.Plan(c.model).diff_bands()
            assert bands and not any(b[2] for b in bands.values()), (c.name, bands)


def test_a_257_x_256_factor_is_beyond_the_generic_kernel(probe_lib):
    """the named refusal: the updated 257 x 256 factor is planned into the generic class with a dual of 513 doubles, one more than
    GEN_MAXD — the engine refuses the model in set_reparametrization (asserted on the device in the GPU file; never run)"""
    src = open(os.path.join(H.CSRC, "kernels.hpp")).read()
    gen_maxd = int(re.search(r"constexpr int GEN_MAXD = (\d+);", src).group(1))
    m = PR.refused_model()
    assert int(m.f_dim0[2]) + int(m.f_dim1[2]) == gen_maxd + 1
    for d in (M.FORWARD, M.BACKWARD):
        assert E.Plan(m).schedule_classes(d, M.REPAM_ANISOTROPIC).get("generic", 0) >= 1


# ---------------------------------------------------------------------------------------------------------------------------
# 5. planner facts

def _structures():
    """one case per (structure, schedule, computes, label counts): the planner does not look at the values"""
    seen = {}
    for c in PR.CASES:
        seen.setdefault((c.kind, c.d0, c.d1, c.struct, c.sched, c.computes), c)
    return list(seen.values())


def test_a_self_rounding_record_comes_after_its_unaries_and_alone_among_their_factors():
    """Plan alone: a pairwise record that rounds itself sits in a later level than every record of its unaries that precedes it
    in the update order (it reads their labels), and two pairwise records that share a unary are never in one level (both may
    label it)"""
    n = 0
    for c in _structures():
        m = c.model
        plan = E.Plan(m)
        side_unary, _ = PR.links(m)
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            for d in (M.FORWARD, M.BACKWARD):
                upd, lev = plan.update_order(d), plan.update_levels(d, mode)
                pos = {int(f): k for k, f in enumerate(upd)}
                users = {}
                for f in upd:
                    f = int(f)
                    if m.f_kind[f] == M.F_VECTOR:
                        continue
                    for s in (0, 1):
                        u = side_unary.get((f, s))
                        if u is None:
                            continue
                        if u in pos and pos[u] < pos[f]:
                            assert lev[pos[u]] < lev[pos[f]], (c.name, mode, d, u, f)
                        for g in users.get(u, ()):
                            assert lev[pos[g]] != lev[pos[f]], (c.name, mode, d, u, g, f)
                        users.setdefault(u, []).append(f)
                    n += 1
    assert n > 1000


def test_planned_schedules_of_the_new_models_are_hazard_free(probe_lib):
    """tests/schedule_hazards.py models "a pairwise factor that rounds itself touches all its unaries": its checker on the
    forward and the backward sweep of every structure of the list, in both execution forms"""
    failures, pairs = [], 0
    for c in _structures():
        m = c.model
        mi = H.ModelInfo(m)
        o = Oracle(mi.oracle_model)
        probe = H.Probe(probe_lib, m)
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            o.set_reparametrization(mode)
            for d in (M.FORWARD, M.BACKWARD):
                oo, om = o.omega(d, mode)
                mo, mk = o.mask(d, mode)
                S_ = probe.plan([(o.update_order(d), oo, om, mo, mk)], fuse=False)
                v = H.check_all(S_, H.sequence_of(mi, S_))
                pairs += v.stats["pairs"]
                if v:
                    failures.append("%s | mode %d | direction %d: %d violations, first %r" % (c.name, mode, d, len(v), v[:2]))
    assert not failures, "\n".join(failures[:20])
    assert pairs > 10000
