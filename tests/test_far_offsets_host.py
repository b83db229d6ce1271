"""The planner at far offsets (no GPU): the schedule of ``pad_front(m)`` — tens of thousands of isolated padding factors in front of
a small model, tests/far_offset_cases.py — is the schedule of ``m`` field for field, with every dual / const offset moved by
exactly the padding, as Python ints past 2^31 (P31) and 2^32 (P32).  Read through tests/cpp/schedule_probe.cpp: records, ops and
the packet copies of both.  If a GPU test of tests/test_far_offsets_gpu.py fails, this module tells whether the planner or the
kernel is wrong.  The plans of the calls around the sweeps are pinned here as well: which form the joined passes take, the bodies of
the level loop, and the decode plan, which exists behind VECTOR padding only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import far_offset_cases as F                     # noqa: E402
import schedule_hazards as H                     # noqa: E402
from lp_mp_amd import engine as E                # noqa: E402
from lp_mp_amd import model as M                 # noqa: E402
from oracle.binding import Oracle                # noqa: E402

MODES = (M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2, M.REPAM_UNIFORM, M.REPAM_DAMPED_UNIFORM)
PLACEMENTS = ("P31", "P32")
# fields that must be equal as they are; rec_factor / op_peer move by the number of padding factors; offsets: below
SAME = ("rec_launch", "rec_level", "rec_class", "rec_n_recv", "rec_n_send", "rec_op_begin", "rec_kind_flags",
        "op_side", "op_role", "op_code", "op_pad", "op_omega_bits", "op_mailbox_row") + H._LAUNCH + H._CHAIN


@pytest.fixture(scope="module")
def probe_lib(tmp_path_factory):
    return H.build_probe(tmp_path_factory.mktemp("far_probe"))


def _sweeps(m):
    """(name, segments, fuse): directional sweeps and the fused pass of two weight modes, from the oracle on the small model"""
    o = Oracle(F.oracle_model(m))
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        o.set_reparametrization(mode)
        seg = []
        for d in (0, 1):
            oo, om = o.omega(d, mode)
            mo, mk = o.mask(d, mode)
            seg.append((o.update_order(d), oo, om, mo, mk))
        yield "forward %d" % mode, [seg[0]], False
        yield "backward %d" % mode, [seg[1]], False
        yield "pass %d" % mode, seg, True


def _shifted(segs, n_pad):
    return [((np.asarray(s[0], np.int64) + n_pad).astype(np.int32),) + tuple(s[1:]) for s in segs]


def test_pad_sizes_are_the_placements():
    c, d = F.pad_sizes(F.N_PAD["P31"], "dense")
    assert c == 2**31 and d == 2**31 + 32768 and c % 2 == 0 and d % 2 == 0
    c, d = F.pad_sizes(F.N_PAD["P32"], "dense")
    assert c == 2**32 and d == 2**32 + 65536
    assert F.pad_sizes(F.N_PAD["P31"], "vector") == (0, 2**31)


@pytest.mark.parametrize("kind", ["dense", "vector"])
def test_pad_front_is_the_model_behind_isolated_factors(kind):
    m = F.live("mixed_graph")
    n = 1000
    far = F.pad_front(m, n, kind)
    assert far.const_data is None and far.dual_data is None and far.n_factors == m.n_factors + n
    for a in ("f_type", "f_kind", "f_flags", "f_dim0", "f_dim1", "f_table"):
        assert np.array_equal(getattr(far, a)[n:], getattr(m, a)) and getattr(far, a).dtype == getattr(m, a).dtype, a
    assert np.all(far.f_table[:n] == -1)
    for a in ("m_left", "m_right", "rel_fwd", "rel_bwd"):
        assert np.array_equal(getattr(far, a), getattr(m, a) + n) and getattr(far, a).shape == getattr(m, a).shape, a
    pc, pd = F.pad_sizes(n, kind)
    assert int(far.const_offsets()[n]) == pc and int(far.dual_offsets()[n]) == pd
    assert np.array_equal(far.const_offsets()[n:] - pc, m.const_offsets()) and np.array_equal(far.dual_offsets()[n:] - pd, m.dual_offsets())
    touched = set(far.m_left.tolist()) | set(far.m_right.tolist()) | set(far.rel_fwd.reshape(-1).tolist())
    assert min(touched) >= n                                   # the padding is isolated
    assert not np.asarray(far.ftype_computes_primal)[far.f_type[:n]].any()
    g = F.live("deep_dense16")
    assert g.part_pairs is None or len(g.part_pairs) == 0
    import diff_tables_cases as DT
    pm = DT.rtype_grid(M.RTYPE_PARTITION)
    assert np.array_equal(F.pad_front(pm, n, kind).part_pairs, pm.part_pairs + n)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", list(F.LIVE))
def test_padding_does_not_change_which_kernel_runs(name, placement):
    m = F.live(name)
    far = F.pad_front(m, F.N_PAD[placement], "dense")
    a, b = E.Plan(m), E.Plan(far)
    for mode in MODES:
        for d in (0, 1):
            ca = a.schedule_classes(d, mode)
            assert ca == b.schedule_classes(d, mode), (mode, d)
            want = F.LIVE[name][1]
            if want:
                assert set(ca) == want, (mode, d, ca)
            elif d == 1:      # the op-by-op classes: one wave (generic) or one lane (small) per factor, or the updated pairwise factors
                assert set(ca) & {"generic", "small", "pairwise8"}, ca
        ia, ib = a.schedule_info(0, mode), b.schedule_info(0, mode)
        assert ia == ib, (mode, ia, ib)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", list(F.LIVE))
def test_far_schedule_is_the_small_schedule_moved_by_the_padding(probe_lib, name, placement):
    m = F.live(name)
    n_pad = F.N_PAD[placement]
    pad_c, pad_d = F.pad_sizes(n_pad, "dense")
    assert pad_c >= (2**31 if placement == "P31" else 2**32)
    near, far = H.Probe(probe_lib, m), H.Probe(probe_lib, F.pad_front(m, n_pad, "dense"))
    vector = (m.f_kind == M.F_VECTOR).tolist()
    coff, doff = m.const_offsets().tolist(), m.dual_offsets().tolist()
    NOP = H.NO_PACKET
    packets = 0
    for sname, segs, fuse in _sweeps(m):
        A, B = near.plan(segs, fuse), far.plan(_shifted(segs, n_pad), fuse)
        for k in SAME:
            assert np.array_equal(A[k], B[k]), (sname, k)
        assert len(A["chains"]) == len(B["chains"])
        for ca, cb in zip(A["chains"], B["chains"]):
            for k in H._PER_CHAIN:
                assert np.array_equal(ca[k], cb[k]), (sname, k)      # tickets and dependencies
        assert np.array_equal(A["rec_factor"] + n_pad, B["rec_factor"]) and np.array_equal(A["op_peer"] + n_pad, B["op_peer"]), sname
        assert len(A["rec_factor"]) > 0
        fa = A["rec_factor"].tolist()
        # records: own dual start, own const start (-1: a vector factor), and the same words of the packet header
        for rk, pk, off, pad in (("rec_dual_off", "pk_rec_dual_off", doff, pad_d), ("rec_const_off", "pk_rec_const_off", coff, pad_c)):
            a, b, pa, pb = A[rk].tolist(), B[rk].tolist(), A[pk].tolist(), B[pk].tolist()
            for i, f in enumerate(fa):
                want = -1 if (rk == "rec_const_off" and vector[f]) else off[f]
                assert a[i] == want and b[i] == (want if want == -1 else want + pad), (sname, rk, i, a[i], b[i])
                assert (pa[i] == NOP) == (pb[i] == NOP) and (pa[i] == NOP or (pa[i] == a[i] and pb[i] == b[i])), (sname, pk, i)
                packets += pa[i] != NOP
        # ops: the peer's dual start always moves; the peer's const start moves when it is one (a unary-pairwise message seen from
        # the left): -1 (seen from the right), a labeling-table offset and the 0 of a min-norm message stay
        code, role, peer, row = A["op_code"].tolist(), A["op_role"].tolist(), A["op_peer"].tolist(), A["op_mailbox_row"].tolist()
        a, b, pa, pb = (X[k].tolist() for k in ("op_peer_dual", "pk_op_peer_dual") for X in (A, B))
        ac, bc, pac, pbc = (X[k].tolist() for k in ("op_peer_const", "pk_op_peer_const") for X in (A, B))
        n_recv_of = {}
        for i in range(len(fa)):
            for k in range(A["rec_n_recv"][i] + A["rec_n_send"][i]):
                n_recv_of[int(A["rec_op_begin"][i]) + k] = k < A["rec_n_recv"][i]
        for o in range(len(code)):
            assert a[o] == doff[peer[o]] and b[o] == a[o] + pad_d, (sname, "op_peer_dual", o)
            assert (pa[o] == NOP) == (pb[o] == NOP) and (pa[o] == NOP or (pa[o] == a[o] and pb[o] == b[o])), (sname, "pk_op_peer_dual", o)
            is_const = code[o] == M.M_UNARY_PAIRWISE and role[o] == 0
            if is_const:
                assert ac[o] == coff[peer[o]] and bc[o] == ac[o] + pad_c, (sname, "op_peer_const", o)
            else:
                assert bc[o] == ac[o] and (code[o] != M.M_UNARY_PAIRWISE or ac[o] == -1), (sname, "op_peer_const unshifted", o, ac[o], bc[o])
            assert (pac[o] == NOP) == (pbc[o] == NOP)
            if pac[o] != NOP:
                if row[o] >= 0 and not n_recv_of[o]:           # a mailbox send: the packet word is the row
                    assert pac[o] == row[o] and pbc[o] == row[o]
                else:
                    assert pac[o] == ac[o] and pbc[o] == bc[o], (sname, "pk_op_peer_const", o)
        assert all(type(x) is int for x in b[:1] + bc[:1])
        assert min(b) >= pad_d
        if name == "level_loop40":                                 # the model of the level-loop test: one workgroup walks its launches
            assert B["chain_level_loop"].tolist() == [1], sname
    if F.LIVE[name][1] and not F.LIVE[name][1] & {"dense_big", "diff"}:
        assert packets > 0, "a packed class without packets: the probe did not reach them"


# ---- the models added for the kernels that came after the first far-offset tests ---------------------------------------------
SMALL_NEW_MODELS = F.DIFF_SHIFT_MODELS + ("pq_mixed_sides",) + tuple(F.LABELING_NL)
NEW_MODELS = SMALL_NEW_MODELS + F.DIFF_SHIFT_BAND_MODELS + ("skew_dense32",)
DECODE_MODELS = ("dense8", "dense_v21", "big130", "shared32", "diff_shift40")
ERR_UNSUPPORTED = -2


def test_new_models_are_what_the_gpu_tests_take_them_for():
    """kinds, label counts and sizes (at most 270 k constants and 66 k duals: TAIL stays), the peer-minima form, and the bodies of
    the level loop the two labeling models reach — on the SMALL plans; the far plans equal them in the test below"""
    import labeling_cases as LC
    ANISO = M.REPAM_ANISOTROPIC
    for name in SMALL_NEW_MODELS:
        m = F.live(name)
        assert int(m.const_sizes().sum()) <= 270_000 and m.dual_data.shape[0] <= 66_000, name
    # the banded DIFF_SHIFT grids: every vector inside the rule (the numpy statement), every shifted launch of the plan banded, and
    # the second with more than 128 labels (the LDS-bound occupancy branch of the banded kernel)
    import diff_shift_band_cases as DB
    for name, L in (("diff_shift_band40", 40), ("diff_shift_band130", 130)):
        m = F.live(name)
        assert set(m.f_kind.tolist()) == {M.F_VECTOR, M.F_PAIRWISE_DIFF_SHIFT} and set(m.f_dim0[m.f_kind == M.F_VECTOR].tolist()) == {L}
        assert DB.banded(m), name
        p = E.Plan(m)
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            for d in (0, 1):
                i = p.diff_shift_band_info(d, mode)
                assert i["shift_band_launches"] == i["shift_launches"] > 0, (name, mode, d, i)
    # the grid of the skewed tiled order: 24 x 24 of 32 labels, joined passes in the peer-minima form
    m = F.live("skew_dense32")
    assert int((m.f_kind == M.F_VECTOR).sum()) == 24 * 24 and set(m.f_dim0.tolist()) == {32} and set(m.f_dim1[m.f_kind != M.F_VECTOR].tolist()) == {32}
    p = E.Plan(m)
    assert p.pass_rotates(ANISO) and p.peer_minima(ANISO) == (True, "")
    for name, L in (("diff_shift40", 40), ("diff_shift130", 130)):
        m = F.live(name)
        assert set(m.f_kind.tolist()) == {M.F_VECTOR, M.F_PAIRWISE_DIFF_SHIFT} and set(m.f_dim0[m.f_kind == M.F_VECTOR].tolist()) == {L}
    mixed = F.live("diff_shift_mixed")
    assert {M.F_PAIRWISE_DIFF_SHIFT, M.F_PAIRWISE_DIFF, M.F_PAIRWISE_SHARED, M.F_PAIRWISE_DENSE, M.F_PAIRWISE_POTTS} <= set(mixed.f_kind.tolist())
    p = E.Plan(F.live("pq_mixed_sides"))
    assert p.pass_rotates(ANISO) and p.peer_minima(ANISO) == (True, "")
    assert E.Plan(F.live("joined_dense32")).peer_minima(ANISO) == (True, "")
    for name, cls in (("labeling_nl_small", "small"), ("labeling_nl_generic", "generic")):
        c = LC.CASES[F.LABELING_NL[name]]
        assert c.fam.cls == cls and c.fam.nl > 1 and c.chain_min == 0, name
        p = E.Plan(F.live(name))
        for mode in MODES:
            for d in (0, 1):
                assert set(p.schedule_classes(d, mode)) == {cls}, (name, mode, d)
    assert LC.CASES[F.LABELING_NL["labeling_nl_generic"]].fam.nl >= 9
    p = E.Plan(F.live("labeling_nl_small"))
    reached = {b for d in (0, 1, -1) for mode in MODES for b, n in LC.bodies(p, d, mode).items() if n > 0}
    assert {"paired staged", "staged"} <= reached, reached


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", NEW_MODELS)
def test_new_models_plan_alike_behind_the_padding(name, placement):
    """class sets, whether passes join, the peer-minima form, the shifted launches of class diff and the bodies of the level loop:
    the far plan's equal the small plan's"""
    import labeling_cases as LC
    m = F.live(name)
    a, b = E.Plan(m), E.Plan(F.pad_front(m, F.N_PAD[placement], "dense"))
    for mode in MODES:
        for d in (0, 1):
            assert a.schedule_classes(d, mode) == b.schedule_classes(d, mode), (mode, d)
            assert a.diff_band_info(d, mode) == b.diff_band_info(d, mode), (mode, d)
            assert a.diff_shift_band_info(d, mode) == b.diff_shift_band_info(d, mode), (mode, d)
        assert a.pass_rotates(mode) == b.pass_rotates(mode), mode
        assert a.peer_minima(mode) == b.peer_minima(mode), mode
        assert a.pass_schedule_info(mode) == b.pass_schedule_info(mode), mode
        for d in (0, 1, -1):
            assert a.chain_info(d, mode) == b.chain_info(d, mode), (mode, d)
            assert a.level_loop_info(d, mode) == b.level_loop_info(d, mode), (mode, d)
            if name in F.LABELING_NL:
                assert LC.bodies(a, d, mode) == LC.bodies(b, d, mode), (mode, d)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", DECODE_MODELS)
def test_decode_plan_behind_vector_padding(name, placement):
    """the decode planner takes isolated VECTOR factors (each a unary of level 1 without links) and refuses isolated pairwise ones, so
    the far decode runs behind vector padding: far duals, near constants.  Its plan is the small plan's with the padding unaries
    added: as many levels and links, and the live unaries in the same order at the same levels"""
    m = F.live(name)
    n_pad = F.N_PAD[placement]
    a, b = E.Plan(m), E.Plan(F.pad_front(m, n_pad, "vector"))
    for d in (0, 1):
        ia, ib = a.decode_info(d), b.decode_info(d)
        assert ib == dict(n_unaries=ia["n_unaries"] + n_pad, n_levels=ia["n_levels"], n_links=ia["n_links"]), (d, ia, ib)
        assert ia["n_unaries"] == int((m.f_kind == M.F_VECTOR).sum()) and ia["n_levels"] > 1
        (fa, la), (fb, lb) = a.decode_levels(d), b.decode_levels(d)
        live = fb >= n_pad
        assert np.array_equal(fb[live], fa + n_pad) and np.array_equal(lb[live], la), d
        assert sorted(fb[~live].tolist()) == list(range(n_pad)) and np.all(lb[~live] == 1), d
    with pytest.raises(E.EngineError) as ei:
        E.Plan(F.pad_front(m, n_pad, "dense")).decode_info(0)
    assert ei.value.code == ERR_UNSUPPORTED and "factor 0 " in str(ei.value) and "no unary" in str(ei.value), str(ei.value)


# ---- path and forest moves, the primal state: the plans behind the padding, and conditions on the inputs -------------------------
RELABEL_CASES = [(kind, name) for kind in F.RELABEL for name in F.RELABEL[kind]]
ANISO = M.REPAM_ANISOTROPIC


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("kind,name", RELABEL_CASES)
def test_relabel_plans_alike_behind_the_padding(kind, name, placement):
    """lpmp_plan_path_info / lpmp_plan_forest_info: the far plan accepts the groups shifted by the padding and counts what the small
    plan counts — paths, path edges and off-path links; trees, tree edges, off-tree links and the greatest height"""
    m, groups, _ = F.relabel_case(kind, name)
    n_pad = F.N_PAD[placement]
    kw = dict(F.RELABEL[kind][name].kw)
    a, b = E.Plan(m, **kw), E.Plan(F.pad_front(m, n_pad, "dense"), **kw)
    far = F.far_groups(kind, groups, n_pad)
    assert F.relabel_members(kind, far) == [u + n_pad for u in F.relabel_members(kind, groups)] and min(F.relabel_members(kind, far)) >= n_pad
    if kind == "path":
        ia, ib = a.path_info(groups), b.path_info(far)
        assert ia == ib and ia["n_paths"] == sum(len(g) for g in groups) > 0 and ia["n_path_edges"] == sum(len(p) - 1 for g in groups for p in g), (ia, ib)
        assert ia["n_off_path_links"] > 0, ia
    else:
        ia, ib = a.forest_info(groups), b.forest_info(far)
        assert ia == ib and ia["n_trees"] == sum(int((np.asarray(par) == -1).sum()) for _, par in groups) > 0, (ia, ib)
        assert ia["n_tree_edges"] == sum(int((np.asarray(par) != -1).sum()) for _, par in groups) > 0 and ia["max_height"] > 0, ia
        assert ia["n_off_tree_links"] > 0 or name == "thinned_grid", ia          # (the suggested cover of a graph: its groups decide)
    with pytest.raises(E.EngineError):     # the groups as they are name padding factors in the far model: no unaries
        (b.path_info if kind == "path" else b.forest_info)(groups)
    if kind == "forest" and name in ("tree", "diff_shift"):
        for (un, par), (fu, fp) in zip(groups, far):
            assert np.array_equal(fu - n_pad, un) and np.array_equal(fp == -1, np.asarray(par) == -1)


def _host_duals(kind, name):
    """the duals a far GPU test of the case moves on: random ones, or those of the oracle's passes (the engine's, bit for bit: every
    sweep test of the suite asserts it)"""
    c = F.RELABEL[kind][name]
    if not c.passes:
        return F.relabel_random_duals(kind, name)
    o = Oracle(F.oracle_model(F.relabel_case(kind, name)[2])); o.set_reparametrization(ANISO)
    o.ComputePass(c.passes)
    return o.duals().copy()


@pytest.mark.parametrize("kind,name", RELABEL_CASES)
def test_every_relabel_case_moves_a_label_in_its_first_round(kind, name):
    """no far path or forest test can pass vacuously: from the starting labelling the reference changes the label of at least one
    member within the first round (and the labelling it ends on differs from the start)"""
    m, groups, _ = F.relabel_case(kind, name)
    start = F.relabel_start(kind, name)
    trace = []
    want = F.relabel_reference(kind, name, _host_duals(kind, name), start, trace=trace)
    assert len(trace) == F.RELABEL_ROUNDS * len(groups)
    members = F.relabel_members(kind, groups)
    first = trace[len(groups) - 1]
    changed = int(np.sum(first[members, 0] != start[members, 0]))
    print(kind, name, "labels changed in the first round:", changed, "of", len(members))
    assert changed > 0 and not np.array_equal(want, start)


@pytest.mark.parametrize("name", F.CARRY_MODELS)
def test_carried_labels_clamp_somewhere_and_not_everywhere(name):
    """every move of the far carry test: at least one set label leaves its window (it clamps), at least one stays inside, and at
    least one listed unary is unset"""
    m = F.live(name)
    us, L, moves = F.window_moves(name)
    d = m.f_dim0[us].astype(np.int64)
    assert {0, 1, -1, 63, -64, L - 1, -L, L + 7} <= set(moves[0][0].tolist())
    for k, (dl, _, _, labels) in enumerate(moves):
        x = labels[us, 0].astype(np.int64)
        is_set = x < d
        moved = x - dl
        clamped = is_set & ((moved < 0) | (moved > d - 1))
        assert clamped.any() and (is_set & ~clamped).any() and (~is_set).any(), (name, k)
        want = M.move_labels(labels, m, us, dl)
        assert np.array_equal(want[us, 0][clamped], np.where(moved < 0, 0, d - 1)[clamped]) and np.array_equal(want[us, 0][~is_set], d[~is_set]), (name, k)


def test_moves_on_the_banded_model_and_where_it_stays_feasible():
    """diff_shift_band40 has a vector with +inf tails whose band sits on the diagonal.  The four moves of the far window test push it
    off — no finite labelling is left until the windows are back —, so the GPU test compares the bound there and runs no pass; the
    two checkerboard moves behind them change every shift word by one and keep the model feasible, duals finite after the passes.
    The oracle alone, on ``model.move_windows``' models, without passes on an infeasible state — as the GPU test proceeds"""
    import dataclasses
    import move_windows_cases as MW
    name = "diff_shift_band40"
    m = F.live(name)
    us, L, moves = F.window_moves(name)
    more = F.checkerboard_moves(name)
    cells = np.flatnonzero(m.f_kind == M.F_PAIRWISE_DIFF_SHIFT)
    shifts = m.const_data[m.const_offsets()[cells] + 1]
    inner = int((np.abs(shifts) < 2.0 ** 30).sum())                # (a shift at +-2^30 is clipped there: the "huge" placements)
    assert 2 * inner > len(cells)
    o = Oracle(F.oracle_model(m)); o.set_reparametrization(ANISO)
    o.ComputePass(1); o.ComputePass(2)
    d, cur, finite = o.duals().copy(), m, []
    for k, (dl, costs, _, _) in enumerate(moves + more):
        co, cn = MW.cost_pair(cur, us, dl, 12 + k, stride=L + 6) if costs else (None, None)
        m2, d2 = M.move_windows(cur, d, us, dl, co, cn)
        assert np.isfinite(d2).all(), k
        changed = int((m2.const_data != cur.const_data).sum())
        o = Oracle(dataclasses.replace(F.oracle_model(m2), dual_data=np.array(d2, np.float64, copy=True), _keep=[])); o.set_reparametrization(ANISO)
        cur, d = m2, d2
        finite.append(bool(np.isfinite(o.LowerBound())))
        if finite[-1]:
            o.ComputePass(2)
            d = o.duals().copy()
            assert np.isfinite(d).all() and np.isfinite(o.LowerBound()), k
        if k >= len(moves):
            assert finite[-1] and changed >= inner, (k, changed, inner)            # the shift word of every cell inside the clip is rewritten
    print("moves after which the model has a finite labelling:", finite)
    assert finite == [False, True, False, True, True, True]


@pytest.mark.parametrize("name", F.SCALAR_MODELS)
def test_the_send_only_pass_leaves_some_bounds_stale_and_not_all(name):
    """the custom pass of the device-scalar tests: a send marks the tracked bound of its peer stale, so with at least one send-only
    update at least one bound is stale, and the stale bounds lie among the neighbours of the updates kept — fewer than all factors
    (how many exactly the GPU test reads from the engine's counter)"""
    from test_far_offsets_gpu import send_only_updates
    m = F.live(name)
    o = Oracle(F.oracle_model(m)); o.set_reparametrization(ANISO)
    factors = send_only_updates(o, ANISO)[0]
    assert len(factors) > 0
    kept = set(factors.tolist())
    peers = {int(m.m_right[k]) for k in range(m.n_messages) if int(m.m_left[k]) in kept} | {int(m.m_left[k]) for k in range(m.n_messages) if int(m.m_right[k]) in kept}
    assert 0 < len(peers) < m.n_factors, (name, len(peers), m.n_factors)


def test_every_live_model_of_the_relabel_module_fits_the_tail():
    models = [F.live(n) for n in F.DIFF_SHIFT_BAND_MODELS + ("skew_dense32",) + F.SET_LABEL_MODELS + F.CARRY_MODELS + F.SCALAR_MODELS]
    models += [F.relabel_case(kind, name)[0] for kind, name in RELABEL_CASES]
    largest = max(max(int(m.const_data.shape[0]), int(m.dual_data.shape[0])) for m in models)
    print("largest live model: %d doubles of %d" % (largest, F.TAIL))
    assert largest <= F.TAIL
    assert set(F.SET_LABEL_MODELS) <= set(F.LIVE) | set(F.EXTRA) and F.live("primal_shift24").f_kind.tolist().count(M.F_PAIRWISE_DIFF_SHIFT) > 0
