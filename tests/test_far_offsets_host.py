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
NEW_MODELS = F.DIFF_SHIFT_MODELS + ("pq_mixed_sides",) + tuple(F.LABELING_NL)
DECODE_MODELS = ("dense8", "dense_v21", "big130", "shared32", "diff_shift40")
ERR_UNSUPPORTED = -2


def test_new_models_are_what_the_gpu_tests_take_them_for():
    """kinds, label counts and sizes (at most 270 k constants and 66 k duals: TAIL stays), the peer-minima form, and the bodies of
    the level loop the two labeling models reach — on the SMALL plans; the far plans equal them in the test below"""
    import labeling_cases as LC
    ANISO = M.REPAM_ANISOTROPIC
    for name in NEW_MODELS:
        m = F.live(name)
        assert int(m.const_sizes().sum()) <= 270_000 and m.dual_data.shape[0] <= 66_000, name
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
