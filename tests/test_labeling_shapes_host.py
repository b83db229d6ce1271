"""Why the models of tests/labeling_cases.py can tell a wrong labeling kernel from a right one, and which kernel body runs each of
them (CPU only; the device runs are tests/test_labeling_shapes_gpu.py).

1. A reference that is not the oracle.  ``labeling_message<LEFT, RIGHT, INDICES...>`` (reference
   include/factors/labeling_list_factor.hxx:411-506), restated here in plain numpy.  With ``tab[r]`` = the index of the left labeling
   that the right labeling r shows at the index tuple, or nl if it shows none (:384-402), l the left factor's costs and R the right's:
     compute_msg (:411-443)         msg[i] = min_{r: tab[r] == i} R[r] - not_taken,
                                    not_taken = min(0 if the right factor has an implicit origin else +inf, min_{r: tab[r] == nl} R[r])
     send_message_to_left (:479)    the message -= omega * compute_msg(R)
     send_message_to_right (:501)   the message -= omega * l
     RepamLeft (:445-450)           l[i] += delta[i]
     RepamRight (:452-477)          R[r] += delta[tab[r]] for every r with tab[r] < nl
   and ``message -= delta`` (factors_messages.hxx:495-508) adds +delta to the side that did not compute it and -delta to the one that
   did.  The oracle's ``message_value`` and its updates of single factors must equal this bit for bit on every family, and the
   hand-computed values below pin both.  (The header itself cannot be compiled into a checker here: it includes config.hxx, which
   needs the tclap and simdpp headers that are not part of the reference tree; no stand-ins are written.)
2. The two conditions that keep the duals finite (labeling_cases.py: a, b) hold for the tables of every case, and the oracle's
   duals are finite after every call sequence of the device tests.  9 left against 8 right labelings cannot meet (a).
3. The census: which body of level_loop_kernel<1> runs the launches of every case (Plan.level_loop_info), asserted cell by cell.
4. Every small family can tell: two swapped entries of one match table, or the table of nl = 1 in its place, change the oracle's
   duals.
5. lp.py builds the same tables and the same FlatModel from labeling_factor / labeling_message with several indices."""
import numpy as np
import pytest

from lp_mp_amd import model as M
from lp_mp_amd import engine as E
from lp_mp_amd import lp as LP
from oracle.binding import Oracle

import labeling_cases as LC

INF = np.inf
OMEGAS = (1.0, 0.5, 0.3, 1.0 / 3.0)


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------
def np_compute_msg(tab, nl, R, right_implicit_origin):
    not_taken = 0.0 if right_implicit_origin else INF
    msg = np.full(nl, INF)
    for r in range(len(tab)):
        if tab[r] < nl:
            msg[tab[r]] = min(msg[tab[r]], R[r])
        else:
            not_taken = min(not_taken, R[r])
    return msg - not_taken


def np_delta(m, off, duals, msg, to_left, src, omega):
    """omega * (what the computing side sends): by the right factor (to_left) or by the left one"""
    t = m.mtypes[m.m_type[msg]]
    nl = int(m.f_dim0[m.m_left[msg]])
    if to_left:
        tab = m.tab_data[m.tab_off[t.param]: m.tab_off[t.param + 1]]
        assert int(m.tab_nleft[t.param]) == nl
        return np.float64(omega) * np_compute_msg(tab, nl, src, bool(m.f_flags[m.m_right[msg]] & M.FF_IMPLICIT_ORIGIN))
    return np.float64(omega) * np.asarray(src, np.float64)[:nl]


def np_apply(m, off, duals, msg, computed_by_right, delta):
    t = m.mtypes[m.m_type[msg]]
    l, r = int(m.m_left[msg]), int(m.m_right[msg])
    tab = m.tab_data[m.tab_off[t.param]: m.tab_off[t.param + 1]]
    nl = len(delta)
    s = 1.0 if computed_by_right else -1.0

    def left():
        duals[off[l]: off[l] + nl] += s * delta

    def right():
        for j in range(len(tab)):
            if tab[j] < nl:
                duals[off[r] + j] += -s * delta[tab[j]]
    if computed_by_right:
        left(); right()
    else:
        right(); left()


CAPS = {M.SCHED_LEFT: (0, 1, 0, 1), M.SCHED_RIGHT: (1, 0, 1, 0), M.SCHED_FULL: (1, 1, 1, 1), M.SCHED_ONLY_SEND: (1, 1, 0, 0)}   # to_left, to_right, from_left, from_right


def np_update_factor(m, duals, f, entries, om, mk):
    """one factor update under the shared send rule (reference LP_MP.h, UpdateFactor): the masked receives in message-list order,
    each computed by the peer with weight 1; then the sends, all computed from the state after the receives"""
    off = m.dual_offsets()
    ir = 0
    for x in entries:
        msg, role = int(x) // 2, int(x) % 2
        c = CAPS[m.mtypes[m.m_type[msg]].schedule]
        if (c[3] if role == 0 else c[2]):
            if mk[ir]:
                peer = int(m.m_right[msg]) if role == 0 else int(m.m_left[msg])
                by_right = role == 0
                np_apply(m, off, duals, msg, by_right, np_delta(m, off, duals, msg, by_right, duals[off[peer]: off[peer + 1]].copy(), 1.0))
            ir += 1
    snap = duals[off[f]: off[f + 1]].copy()
    i_s = 0
    for x in entries:
        msg, role = int(x) // 2, int(x) % 2
        c = CAPS[m.mtypes[m.m_type[msg]].schedule]
        if (c[1] if role == 0 else c[0]):
            if om[i_s] != 0.0:
                by_right = role == 1
                np_apply(m, off, duals, msg, by_right, np_delta(m, off, duals, msg, by_right, snap, om[i_s]))
            i_s += 1
    assert ir == len(mk) and i_s == len(om)


FAMILY_CASES = {f.name: next(c for c in LC.CASES.values() if c.family == f.name and c.shape == "chain") for f in LC.FAMILIES.values()}


@pytest.mark.parametrize("fam", list(LC.FAMILIES))
def test_oracle_message_values_equal_the_numpy_restatement(fam):
    c = FAMILY_CASES[fam]
    m = LC.build(c)
    o = Oracle(m)
    off, d = m.dual_offsets(), m.dual_data
    for msg in range(m.n_messages):
        l, r = int(m.m_left[msg]), int(m.m_right[msg])
        for omega in OMEGAS:
            want = np_delta(m, off, d, msg, True, d[off[r]: off[r + 1]], omega)
            assert np.all(np.isfinite(want))
            assert np.array_equal(o.message_value(msg, True, omega), want), (fam, msg, omega)
            assert np.array_equal(o.message_value(msg, False, omega), np_delta(m, off, d, msg, False, d[off[l]: off[l + 1]], omega)), (fam, msg, omega)


@pytest.mark.parametrize("fam", list(LC.FAMILIES))
@pytest.mark.parametrize("sched", list(LC.SCHEDS))
def test_oracle_updates_of_one_left_and_one_right_factor_equal_the_numpy_restatement(fam, sched):
    """compute_pass_custom over ONE factor at a time, with random receive masks and send weights: a left factor, then a right one,
    three rounds on the evolving duals"""
    c0 = FAMILY_CASES[fam]
    c = LC.Case(c0.name, c0.family, "chain", sched, c0.io)
    m = LC.build(c)
    o = Oracle(m)
    offs, ent = o.msg_lists()
    rng = np.random.default_rng(5)
    n_left = int(np.sum(m.f_type == 0))
    mine = m.dual_data.copy()
    for rnd in range(3):
        for f in (int(rng.integers(n_left)), n_left + int(rng.integers(m.n_factors - n_left))):
            entries = ent[offs[f]: offs[f + 1]]
            caps = [CAPS[m.mtypes[m.m_type[int(x) // 2]].schedule] for x in entries]
            ns = sum(cp[1] if int(x) % 2 == 0 else cp[0] for x, cp in zip(entries, caps))
            nr = sum(cp[3] if int(x) % 2 == 0 else cp[2] for x, cp in zip(entries, caps))
            om = rng.uniform(0.05, 1, ns) * (rng.uniform(size=ns) < 0.8)
            om = om / max(1.0, om.sum() * 1.25)
            mk = (rng.uniform(size=nr) < 0.7).astype(np.uint8)
            o.compute_pass_custom(np.array([f], np.int32), np.array([0, ns], np.int64), om, np.array([0, nr], np.int64), mk)
            np_update_factor(m, mine, f, entries, om, mk)
            assert np.array_equal(o.duals(), mine), (fam, sched, rnd, f)
    assert not np.array_equal(mine, m.dual_data) and np.all(np.isfinite(mine))


def _pair_trip7_single(R, left_costs, rio, lio=False):
    f = LC.FAMILIES["pair_trip7"]
    b = M.ModelBuilder(2, [M.MsgType(0, 1, M.SCHED_LEFT, 0, 0, M.M_LABELING, k) for k in range(3)])
    for k in range(3):
        b.add_labeling_table(f.left, f.right, f.indices[k])
    lf = b.add_vector_factors(0, np.asarray(left_costs, np.float64), implicit_origin=lio)
    rf = b.add_vector_factors(1, np.asarray([R], np.float64), implicit_origin=rio)
    for k in range(3):
        b.add_messages(k, lf[k], rf[0])
    return b.finish()


def test_hand_computed_known_answers_for_pair_trip7():
    """left labelings (0,1), (1,0), (1,1); right labelings 001 010 011 100 101 110 111 with costs R = 5 1 4 2 8 7 3.
    table (0,1): the right labelings show 00 01 01 10 10 11 11 -> tab = 3 0 0 1 1 2 2; not_taken = R[001] = 5;
                 minima 1, 2, 3 -> msg = -4, -3, -2
    table (0,2): they show 01 00 01 10 11 10 11 -> tab = 0 3 0 1 2 1 2; not_taken = R[010] = 1; minima 4, 2, 3 -> msg = 3, 1, 2
    table (1,2): they show 01 10 11 00 01 10 11 -> tab = 0 1 2 3 0 1 2; not_taken = R[100] = 2; minima 5, 1, 3 -> msg = 3, -1, 1
    with an implicit origin on the right factor not_taken = min(0, .) = 0 and the messages are the minima themselves"""
    f = LC.FAMILIES["pair_trip7"]
    assert [t.tolist() for t in f.tables()] == [[3, 0, 0, 1, 1, 2, 2], [0, 3, 0, 1, 2, 1, 2], [0, 1, 2, 3, 0, 1, 2]]
    R = [5.0, 1.0, 4.0, 2.0, 8.0, 7.0, 3.0]
    L = [[10.0, 20.0, 30.0], [1.0, 2.0, 3.0], [0.5, 0.25, 0.125]]
    m = _pair_trip7_single(R, L, rio=False)
    assert m.tab_nleft.tolist() == [3, 3, 3] and m.tab_data.tolist() == [3, 0, 0, 1, 1, 2, 2, 0, 3, 0, 1, 2, 1, 2, 0, 1, 2, 3, 0, 1, 2]
    o = Oracle(m)
    assert o.message_value(0, True).tolist() == [-4.0, -3.0, -2.0]
    assert o.message_value(0, True, 0.5).tolist() == [-2.0, -1.5, -1.0]
    assert o.message_value(1, True).tolist() == [3.0, 1.0, 2.0]
    assert o.message_value(2, True).tolist() == [3.0, -1.0, 1.0]
    assert o.message_value(1, False, 0.5).tolist() == [0.5, 1.0, 1.5]
    oi = Oracle(_pair_trip7_single(R, L, rio=True))
    assert oi.message_value(0, True).tolist() == [1.0, 2.0, 3.0] and oi.message_value(2, True, 0.25).tolist() == [1.25, 0.25, 0.75]
    # the left factor 0 receives through table (0,1) and sends nothing: l += msg, R[r] -= msg[tab[r]] where matched
    one = (np.array([0], np.int32), np.array([0, 1], np.int64), np.array([0.0]), np.array([0, 1], np.int64), np.array([1], np.uint8))
    o.compute_pass_custom(*one)
    d = o.duals()
    assert d[:3].tolist() == [6.0, 17.0, 28.0] and d[9:].tolist() == [5.0, 5.0, 8.0, 5.0, 11.0, 9.0, 5.0]
    # ... then the left factor 1 sends half of itself through table (0,2) without receiving: l -= l / 2, R[r] += (l / 2)[tab[r]]
    o.compute_pass_custom(np.array([1], np.int32), np.array([0, 1], np.int64), np.array([0.5]), np.array([0, 1], np.int64), np.array([0], np.uint8))
    d = o.duals()
    assert d[3:6].tolist() == [0.5, 1.0, 1.5] and d[9:].tolist() == [5.5, 5.0, 8.5, 6.0, 12.5, 10.0, 6.5]
    assert np.array_equal(np_compute_msg(f.tables()[0], 3, np.array(R), False), [-4.0, -3.0, -2.0])


# ---- 2. the two conditions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.CASES))
def test_conditions_a_and_b_hold_for_every_table_of_every_case(name):
    c = LC.CASES[name]
    m = LC.build(c)
    for t in range(len(m.tab_nleft)):
        tab, nl = m.tab_data[m.tab_off[t]: m.tab_off[t + 1]], int(m.tab_nleft[t])
        assert nl == c.fam.nl and len(tab) == c.fam.nr and tab.min() >= 0 and tab.max() <= nl
        assert set(range(nl)) <= set(tab.tolist()), (name, t, "a")
        assert c.io[1] or np.any(tab == nl), (name, t, "b")
    assert m.n_factors <= 400


def _finite(o):
    return bool(np.all(np.isfinite(o.duals())) and np.isfinite(o.LowerBound()))


@pytest.mark.parametrize("name", list(LC.CASES))
def test_oracle_duals_stay_finite_over_the_calls_of_the_device_tests(name):
    from test_fuzz_gpu import random_rows
    c = LC.CASES[name]
    adaptive = c.family in ("pair_trip7", "perm8", "gen9x20")
    for rtype in (M.RTYPE_SHARED, M.RTYPE_RESIDUAL) + ((M.RTYPE_ADAPTIVE,) if adaptive else ()):
        m = LC.build(c, M.MF_IMPROVEMENT if rtype == M.RTYPE_ADAPTIVE else 0)
        for mode in LC.MODES:
            o = Oracle(m)
            o.set_reparametrization_type(rtype); o.set_reparametrization(mode)
            for what, n in LC.CALLS:
                LC.call(o, what, n)
                assert _finite(o), (name, rtype, mode, what, n)
    o = Oracle(m)
    rng = np.random.default_rng(sum(map(ord, name)))
    for k in range(4):
        o.compute_pass_custom(*random_rows(rng, None, o, LC.build(c)))
        assert _finite(o), (name, "random rows", k)


def test_nine_left_labelings_cannot_all_be_matched_by_eight_right_ones():
    """the family 9 x 8 of the issue: whatever the tables hold, one left labeling has no match, its message entry is +inf
    (compute_msg) and the duals are not finite after one pass — in the reference as in the oracle.  So no such case exists; the
    generic class with nl = 9 is covered by 9 x 9 and 9 x 20."""
    f = LC.FAMILIES["gen9x9"]
    c = FAMILY_CASES["gen9x9"]
    tabs = LC.impossible_9x8_tables()
    assert all(len(set(t.tolist())) < 9 for t in tabs)
    b = M.ModelBuilder(2, [M.MsgType(0, 1, M.SCHED_LEFT, 0, 0, M.M_LABELING, k) for k in range(2)])
    for k in range(2):
        b.add_labeling_table(f.left, f.right[:8], f.indices[k])
    b._tables = tabs
    rng = np.random.default_rng(1)
    lf = b.add_vector_factors(0, rng.uniform(-1, 1, (3, 9)))
    rf = b.add_vector_factors(1, rng.uniform(-1, 1, (2, 8)), implicit_origin=True)
    for t in range(2):
        for k in range(2):
            b.add_messages(k, lf[t + k], rf[t]); b.add_relations(lf[t + k], rf[t])
    m = b.finish()
    assert E.Plan(m).schedule_classes(M.BACKWARD, M.REPAM_UNIFORM) == {"generic": 3}
    o = Oracle(m)
    o.set_reparametrization(M.REPAM_UNIFORM)
    assert np.isinf(o.message_value(0, True)).any()
    o.ComputePass(1)
    assert not np.all(np.isfinite(o.duals()))
    assert c.fam.nl == 9


# ---- 3. the census ------------------------------------------------------------------------------------------------------------
def _plan(c, monkeypatch, env=None):
    for k in ("LPMP_NO_LEVEL_LOOP", "LPMP_CHAIN_ALL", "LPMP_CHAIN_MIN", "LPMP_NO_CHAIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        if k != "LPMP_NO_CHAIN":
            monkeypatch.setenv(k, v)
    if c.chain_min:
        monkeypatch.setenv("LPMP_CHAIN_MIN", str(c.chain_min))
    return E.Plan(LC.build(c))


@pytest.mark.parametrize("which", [w for w, _ in LC.ENGINES])
def test_every_case_takes_the_path_of_each_of_the_four_engines(which, monkeypatch):
    """the class split (nothing but the family's class), and: a level loop by default, no chain under LPMP_NO_LEVEL_LOOP, tickets
    under LPMP_CHAIN_ALL"""
    for c in LC.CASES.values():
        LC.assert_path(_plan(c, monkeypatch, dict(LC.ENGINES)[which]), c, which)


def test_the_census_of_kernel_bodies_has_no_empty_cell(monkeypatch):
    """case -> class, bodies of level_loop_kernel<1> over both sweeps and the fused pass of all four modes, nl, nr"""
    reached = {b: set() for b in LC.BODIES}          # body -> the nl that reach it
    rows = []
    for c in LC.CASES.values():
        p = _plan(c, monkeypatch)
        LC.assert_path(p, c, "level loop")
        total = dict.fromkeys(LC.BODIES, 0)
        for mode in LC.MODES:
            for d in (M.FORWARD, M.BACKWARD, -1):
                for b, n in LC.bodies(p, d, mode).items():
                    total[b] += n
        if c.fam.cls == "small":
            for b, n in total.items():
                if n:
                    reached[b].add(c.fam.nl)
        else:
            assert sum(total.values()) == 0, c.name
        rows.append((c.name, c.fam.cls, c.fam.nl, c.fam.nr, [total[b] for b in LC.BODIES]))
    print("\n%-38s %-8s %3s %4s  %s" % ("case", "class", "nl", "nr", " | ".join(LC.BODIES)))           # (shown with pytest -s)
    for r in rows:
        print("%-38s %-8s %3d %4d  %s" % (r[0], r[1], r[2], r[3], " | ".join("%d" % x for x in r[4])))
    small = LC.SMALL_CASES
    # each lane-per-op body and the fallback, by a family with several left labelings — and by the control
    for b in LC.BODIES:
        assert reached[b] - {1}, (b, reached[b])
        assert 1 in reached[b], (b, reached[b])
    assert reached["paired staged"] >= {1, 2, 3, 4, 8} and reached["staged"] >= {1, 2, 3, 4, 8}
    assert reached["paired"] >= {2, 3, 4, 8} and reached["plain"] >= {2, 3, 4, 8}
    # the fallback inside the loop: nine receives, and two receives on one peer
    assert {c.shape for c in small if c.shape.startswith("hub") or c.shape == "dup"} == {"hub8", "hub9", "dup"}
    for c in small:
        if c.shape in ("hub8", "hub9", "dup") and c.sched == "left":
            n = LC.bodies(_plan(c, monkeypatch), M.BACKWARD, M.REPAM_UNIFORM)["lane per factor"]
            assert n == (0 if c.shape == "hub8" else 1), (c.name, n)
    # role 0 and role 1: under schedule left only left factors are updated, under right only right ones (generic_body<1>)
    for c in small:
        if c.shape == "chain" and c.sched in ("left", "right") and c.io == c.fam.io:
            b = LC.bodies(_plan(c, monkeypatch), M.BACKWARD, M.REPAM_UNIFORM)
            assert (b["lane per factor"] == 0) == (c.sched == "left") and sum(b.values()) > 0, (c.name, b)
    assert {c.sched for c in small} == set(LC.SCHEDS)
    assert {c.fam.nl for c in small} == {1, 2, 3, 4, 8} and {c.fam.nr for c in small} == {4, 7, 8}
    unmatched = {c.family: any(np.any(t == c.fam.nl) for t in c.fam.tables()) for c in small}
    assert set(unmatched.values()) == {True, False}, unmatched
    t0, t1 = LC.FAMILIES["perm8"].tables()
    assert t0.tolist() == list(range(8)) and sorted(t1.tolist()) == list(range(8)) and np.any(np.diff(t1) < 0) and t1.tolist() != t0.tolist()
    # staged / unstaged edge: 16 records is the last staged count, 17 the first that reads its records from memory
    for k, staged in ((16, True), (17, False)):
        i = _plan(LC.CASES["pair_trip7 copies%d left io11" % k], monkeypatch).level_loop_info(M.BACKWARD, M.REPAM_UNIFORM)
        assert i["label_ops"] == i["launches"] > 0 and i["label_staged"] == (i["label_ops"] if staged else 0), (k, i)
    # every combination of the implicit-origin flags
    assert {c.io for c in small} == {(False, False), (False, True), (True, False), (True, True)}
    # the generic class: every family
    assert {c.family for c in LC.GENERIC_CASES} == {f.name for f in LC.GENERIC}
    for c in LC.GENERIC_CASES:
        if c.family == "gen200x512":
            assert c.sched in ("right", "full") and c.fam.nr == LC.GEN_MAXD
    assert LC.FAMILIES["gen5x600"].nr > LC.GEN_MAXD and LC.FAMILIES["gen65x200"].nl % 64 == 1


def test_level_loop_info_agrees_with_the_constants_and_counts_nothing_without_a_loop(monkeypatch):
    monkeypatch.setenv("LPMP_CHAIN_MIN", "2")
    p = E.Plan(LC.case("perm8 copies17 left io01"))
    i = p.level_loop_info(M.BACKWARD, M.REPAM_ANISOTROPIC)
    assert i == dict(launches=5, lane_launches=5, label_ops=5, label_paired=1, label_staged=0, label_paired_staged=0)
    monkeypatch.setenv("LPMP_NO_LEVEL_LOOP", "1")
    q = E.Plan(LC.case("perm8 copies17 left io01"))
    assert set(q.level_loop_info(M.BACKWARD, M.REPAM_ANISOTROPIC).values()) == {0}
    with pytest.raises(E.EngineError):
        p.level_loop_info(2, M.REPAM_ANISOTROPIC)
    import os
    import re
    src = open(os.path.join(os.path.dirname(E.__file__), "csrc", "plan.hpp")).read()
    assert re.search(r"LL_STAGE_RECS = %d, LL_STAGE_OPS = %d;" % (LC.LL_STAGE_RECS, LC.LL_STAGE_OPS), src)
    assert "LL_STAGE_RECS =" not in open(os.path.join(os.path.dirname(E.__file__), "csrc", "kernels.hip")).read()


# ---- 4. the cases can tell ----------------------------------------------------------------------------------------------------
def _duals_after(m, mode=M.REPAM_UNIFORM):
    o = Oracle(m)
    o.set_reparametrization(mode)
    o.ComputePass(2)
    return o.duals()


@pytest.mark.parametrize("fam", [f.name for f in LC.SMALL])
def test_a_wrong_match_table_changes_the_duals(fam):
    c = FAMILY_CASES[fam]
    f = c.fam
    want = _duals_after(LC.build(c))
    assert np.all(np.isfinite(want))
    for k, t in enumerate(f.tables()):
        i, j = next((i, j) for i in range(f.nr) for j in range(i + 1, f.nr) if t[i] != t[j])
        tabs = [u.copy() for u in f.tables()]
        tabs[k][[i, j]] = tabs[k][[j, i]]
        assert not np.array_equal(_duals_after(LC.build(c, tables=tabs)), want), (fam, k, "swapped", i, j)
        if f.nl > 1:                    # every match reads left labeling 0, as all tables of one left labeling do
            tabs = [u.copy() for u in f.tables()]
            tabs[k] = np.where(tabs[k] < f.nl, 0, f.nl).astype(np.int32)
            assert not np.array_equal(_duals_after(LC.build(c, tables=tabs)), want), (fam, k, "nl = 1")


# ---- 5. the mirror ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["pair_trip7", "pair4_trip8", "perm8", "many_to_one", "gen9x20"])
def test_lp_mirror_builds_the_same_model(fam):
    c = FAMILY_CASES[fam]
    f = c.fam
    want = LC.build(c)
    T = len(f.indices)
    FL = LP.FactorContainer(LP.labeling_factor(f.left, c.io[0]), 0)
    FR = LP.FactorContainer(LP.labeling_factor(f.right, c.io[1]), 1)
    ML = [LP.MessageContainer(LP.labeling_message(f.left, f.right, f.indices[k]), 0, 1, LC.SCHEDS[c.sched], 0, 0, k) for k in range(T)]
    lp = LP.LP(LP.FMC("labeling shapes", [FL, FR], ML))
    n_left, n_right, edges = c.graph()
    off = want.dual_offsets()
    ids = [lp.add_factor(FL, want.dual_data[off[i]: off[i + 1]]) for i in range(n_left)]
    ids += [lp.add_factor(FR, want.dual_data[off[n_left + i]: off[n_left + i + 1]]) for i in range(n_right)]
    for a, r, k in edges:
        lp.add_message(ML[k], ids[a], ids[n_left + r])
        lp.AddFactorRelation(ids[a], ids[n_left + r])
    lp.add_to_constant(want.constant)
    got = lp.flat_model()
    assert len(f.indices[0]) >= 1 and (fam == "many_to_one" or len(f.indices[0]) >= 2)
    for k in ("tab_off", "tab_data", "tab_nleft", "f_type", "f_kind", "f_flags", "f_dim0", "f_dim1", "dual_data", "m_type", "m_left", "m_right", "rel_fwd", "rel_bwd"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), (fam, k)
    assert got.mtypes == want.mtypes and got.constant == want.constant and got.n_ftypes == want.n_ftypes
    assert [t.tolist() for t in f.tables()] == [got.tab_data[got.tab_off[k]: got.tab_off[k + 1]].tolist() for k in range(T)]
