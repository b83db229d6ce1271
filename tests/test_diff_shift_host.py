"""Shifted difference-indexed pairwise factors (F_PAIRWISE_DIFF_SHIFT) on the host: model format, expansion, the window property,
validation, the plan and its kernel class — no GPU.  A DIFF_SHIFT factor is bit for bit a DENSE factor whose table is
np.float64(scale) * D[min(max(a - b + s, 0), n - 1)]."""
import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import diff_shift_cases as C

GENERIC = {"generic", "small"}


def _dense_table(D, d0, d1, scale, s):
    n = len(D)
    return np.array([[np.float64(scale) * D[min(max(a - b + s, 0), n - 1)] for b in range(d1)] for a in range(d0)])


def _tables(m):
    """{factor: its d0 x d1 table in expand_diff()} for the difference-indexed factors of m"""
    x = m.expand_diff()
    co = x.const_offsets()
    return {int(f): x.const_data[co[f]:co[f + 1]].reshape(int(m.f_dim0[f]), int(m.f_dim1[f]))
            for f in np.flatnonzero((m.f_kind == M.F_PAIRWISE_DIFF) | (m.f_kind == M.F_PAIRWISE_DIFF_SHIFT))}


def test_builder_sizes_and_expansion_by_plain_loops():
    rng = np.random.default_rng(1)
    b = M.ModelBuilder(3, [M.MsgType(0, 1, param=0), M.MsgType(0, 1, param=1)])
    u = b.add_vector_factors(0, rng.uniform(0, 1, (3, 4)))
    D = [rng.uniform(0, 1, n) for n in (1, 3, 7, 20)]
    t = [b.add_diff_table(v) for v in D]
    scales, shifts = np.array([0.5, 1.75, -2.0, 1.0, 3.0]), np.array([0, 3, -2, 9, -40])
    p = b.add_diff_shift_pairwise(1, 4, 4, [t[2], t[0], t[3], t[1], t[3]], scales, shifts)
    q = b.add_diff_pairwise(1, 4, 4, [t[2]], [0.75])              # one pool entry serves both kinds
    for k in range(2):
        b.add_messages(0, u[k], p[k]); b.add_messages(1, u[k + 1], p[k])
    m = b.finish()
    assert M.F_PAIRWISE_DIFF_SHIFT == 6 and m.has_diff and not m.has_shared
    assert list(m.f_kind[3:]) == [M.F_PAIRWISE_DIFF_SHIFT] * 5 + [M.F_PAIRWISE_DIFF] and list(m.f_table) == [-1] * 3 + [2, 0, 3, 1, 3, 2]
    assert list(m.const_sizes()) == [0, 0, 0, 2, 2, 2, 2, 2, 1] and list(m.dual_sizes()) == [4] * 3 + [8] * 6
    co = m.const_offsets()
    assert np.array_equal(m.const_data[co[3]:co[8]].reshape(5, 2), np.stack([scales, shifts.astype(np.float64)], 1))
    x = m.expand_diff()
    assert not x.has_diff and x.f_table is None and x.n_shared_tables == 0 and set(x.f_kind[3:]) == {M.F_PAIRWISE_DENSE}
    assert np.array_equal(x.dual_data, m.dual_data)
    tab = _tables(m)
    for k, (ti, sc, sh) in enumerate(zip([2, 0, 3, 1, 3], scales, shifts)):
        assert tab[int(p[k])].tobytes() == _dense_table(D[ti], 4, 4, sc, int(sh)).tobytes(), k
    assert tab[int(q[0])].tobytes() == _dense_table(D[2], 4, 4, 0.75, 3).tobytes()
    y = m.expand_shared()                                          # leaves both difference-indexed kinds and their pool alone
    assert y.has_diff and np.array_equal(y.f_table, m.f_table) and np.array_equal(y.const_data, m.const_data)
    # what the builder refuses
    for bad in (0.5, np.nan, np.inf, 2.0 ** 30 + 1, -(2.0 ** 30) - 1):
        with pytest.raises(ValueError):
            b.add_diff_shift_pairwise(1, 4, 4, [t[0]], [1.0], [bad])
    b.add_diff_shift_pairwise(1, 4, 4, [t[0], t[1]], [1.0, 1.0], [2.0 ** 30, -(2.0 ** 30)])
    with pytest.raises(ValueError):
        b.add_diff_shift_pairwise(1, 4, 4, [9], [1.0], [0])
    with pytest.raises(ValueError):
        b.add_diff_shift_pairwise(1, 4, 4, [b.add_shared_table(np.zeros((2, 2)))], [1.0], [0])
    with pytest.raises(ValueError):
        b.add_diff_shift_pairwise(1, 4, 4, [t[0], t[1]], [1.0, 1.0], [0, 1, 2])


def test_shift_conversion_is_the_device_rule():
    """NaN -> 0, saturated to [-2^30, 2^30], truncated toward zero: what expand_diff() does with a shift ModelBuilder would refuse"""
    for x, want in ((np.nan, 0), (np.inf, 1 << 30), (-np.inf, -(1 << 30)), (1e300, 1 << 30), (-3.9, -3), (3.9, 3), (-0.0, 0), (7.0, 7)):
        assert M.diff_shift_int(x) == want, x
    m = C.shift_grid(3, 2, 5, lengths=(4,), shifts=np.zeros(7))
    f = int(np.flatnonzero(m.f_kind == M.F_PAIRWISE_DIFF_SHIFT)[0])
    co = m.const_offsets()
    D = m.shared_table(0).reshape(-1)
    for x in (np.nan, np.inf, -np.inf, -2.5, 1.5):
        m.const_data[co[f] + 1] = x
        assert _tables(m)[f].tobytes() == _dense_table(D, 5, 5, m.const_data[co[f]], M.diff_shift_int(x)).tobytes(), x


def test_the_degenerate_case_is_the_plain_diff_expansion():
    for order in C.ORDERS:
        a, b = C.degenerate_pair(order=order)
        assert np.all(b.f_kind[a.f_kind == M.F_PAIRWISE_DIFF] == M.F_PAIRWISE_DIFF_SHIFT)
        assert a.expand_diff().const_data.tobytes() == b.expand_diff().const_data.tobytes()
    rng = np.random.default_rng(3)
    for d0, d1 in ((3, 7), (7, 3), (1, 5), (6, 1)):
        Dv = rng.uniform(0, 1, d0 + d1 - 1)
        out = []
        for shifted in (False, True):
            b = M.ModelBuilder(2, S.mrf_mtypes())
            b.add_vector_factors(0, np.zeros((1, 2)))
            t = b.add_diff_table(Dv)
            b.add_diff_shift_pairwise(1, d0, d1, [t], [1.5], [d1 - 1]) if shifted else b.add_diff_pairwise(1, d0, d1, [t], [1.5])
            out.append(b.finish().expand_diff().const_data.tobytes())
        assert out[0] == out[1], (d0, d1)


@pytest.mark.parametrize("quadratic", [False, True])
def test_window_property(quadratic):
    """expand(windowed)[a, b] is the full dense table at [a + c_u, b + c_v]: the compact vector has constant tails, so the clamp
    is exact, and the two helpers give the entries of the full-range constructors to the bit"""
    for seed in range(4):
        full, win = 24 + seed, 5 + 2 * seed
        a, w, c = C.window_case(seed=seed, full=full, win=win, quadratic=quadratic)
        assert w.sh_dim1[0] < 2 * full - 1 and a.sh_dim1[0] == 2 * full - 1
        ta, tw = _tables(a), _tables(w)
        for e, f in enumerate(sorted(ta)):
            want = ta[f][c[e]:c[e] + win, c[e + 1]:c[e + 1] + win]
            assert tw[f].tobytes() == np.ascontiguousarray(want).tobytes(), (seed, e)
    Dc, z = (M.truncated_quadratic_compact if quadratic else M.truncated_linear_compact)(0.3, 1.0)
    Df = (M.truncated_quadratic if quadratic else M.truncated_linear)(50, 50, 0.3, 1.0)
    assert len(Dc) == 2 * z + 1 and Dc[0] == Dc[-1] == 1.0 and Dc[1] < 1.0 and Dc[z] == 0.0
    assert Df[49 - z:49 + z + 1].tobytes() == Dc.tobytes() and np.all(Df[:49 - z] == 1.0) and np.all(Df[49 + z + 1:] == 1.0)
    assert int(M.window_shift(7, 3, z)) == 4 + z and list(M.window_shift([1, 2], [2, 0], 1)) == [0, 3]


def _bad(m, **kw):
    import dataclasses
    with pytest.raises(E.EngineError) as ei:
        E.Plan(dataclasses.replace(m, _keep=[], **kw))
    return str(ei.value)


def test_planner_refusals_name_the_factor():
    m = C.shift_grid(3, 2, 5, lengths=(4, 9))
    f = int(np.flatnonzero(m.f_kind == M.F_PAIRWISE_DIFF_SHIFT)[2])
    assert "factor %d" % int(np.flatnonzero(m.f_kind == M.F_PAIRWISE_DIFF_SHIFT)[0]) in _bad(m, f_table=None)
    for t in (-1, 2):
        ft = m.f_table.copy(); ft[f] = t
        msg = _bad(m, f_table=ft)
        assert "factor %d" % f in msg and "out of range" in msg, msg
    d1 = m.f_dim1.copy(); d1[f] = 0
    assert "factor %d" % f in _bad(m, f_dim1=d1)
    # a pool entry that is a table, not a vector
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = b.add_vector_factors(0, np.zeros((2, 3)))
    p = b.add_diff_shift_pairwise(1, 3, 3, [b.add_diff_table(np.arange(6.0))], [1.0], [1])
    b.add_messages(0, u[0], p[0]); b.add_messages(1, u[1], p[0])
    g = b.finish()
    msg = _bad(g, sh_dim0=np.array([2], np.int32), sh_dim1=np.array([3], np.int32))
    assert "factor 2" in msg and "2 x 3" in msg, msg
    # any length is a vector; the plan reads no cost: a shift and a scale of any bits pass
    g.const_data[:] = [np.nan, np.inf]
    E.Plan(g)
    kind = m.f_kind.copy(); kind[f] = 9
    assert "factor %d" % f in _bad(m, f_kind=kind) and "unknown kind" in _bad(m, f_kind=kind)


def test_a_pure_grid_is_class_diff_and_never_banded():
    for L in (3, 40, 130, 512):
        H, W = C.grid_shape(L)
        for order in C.ORDERS:
            p = E.Plan(C.label_grid(L, order))
            for mode in C.MODES:
                for d in (0, 1):
                    assert p.schedule_classes(d, mode) == {"diff": H * W}, (L, order, mode, d)
    m = C.banded_grid()
    p = E.Plan(m)
    assert p.diff_bands() == {}                                     # only DIFF_SHIFT factors reference the entries: -1
    for mode in C.MODES:
        for d in (0, 1):
            assert set(p.schedule_classes(d, mode)) == {"diff"}
            info = p.diff_band_info(d, mode)
            assert info["diff_launches"] > 0 and info["band_launches"] == 0 and info["band_receives"] == 0, info
    # the plain DIFF grid on the same vectors IS banded, and new pool values do not band a shifted launch
    V = [m.shared_table(t).reshape(-1) for t in range(m.n_shared_tables)]
    q = E.Plan(S.grid_model(7, 6, 40, pairwise="diff", order="colour_major", seed=3, diff_tables=np.stack(V)))
    assert q.diff_band_info(0, M.REPAM_ANISOTROPIC)["band_launches"] == q.diff_band_info(0, M.REPAM_ANISOTROPIC)["diff_launches"] > 0
    p.set_shared_pool(m.sh_data * 2.0)
    assert p.diff_band_info(0, M.REPAM_ANISOTROPIC)["band_launches"] == 0


def _two_edges(first, second, L=16):
    """u0 - p0 - u1 - p1 - u2 with pairwise factors of the two given kinds"""
    rng = np.random.default_rng(2)
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = b.add_vector_factors(0, rng.uniform(0, 1, (3, L)))

    def add(kind):
        if kind == "diff_shift":
            return b.add_diff_shift_pairwise(1, L, L, [b.add_diff_table(rng.uniform(0, 1, 9))], [1.5], [3])[0]
        if kind == "diff":
            return b.add_diff_pairwise(1, L, L, [b.add_diff_table(M.truncated_linear(L, L, 0.5, 1.0))], [1.5])[0]
        if kind == "dense":
            return b.add_dense_pairwise(1, rng.uniform(0, 1, (1, L, L)))[0]
        if kind == "potts":
            return b.add_potts_pairwise(1, L, [0.7])[0]
        return b.add_shared_pairwise(1, [b.add_shared_table(rng.uniform(0, 1, (L, L)))], [0.7])[0]
    p0, p1 = add(first), add(second)
    b.add_messages(0, u[0], p0); b.add_messages(1, u[1], p0); b.add_messages(0, u[1], p1); b.add_messages(1, u[2], p1)
    b.add_relations([u[0], p0, u[1], p1], [p0, u[1], p1, u[2]])
    return b.finish()


def test_class_eligibility_beside_other_kinds():
    # one DIFF and one DIFF_SHIFT peer: class diff, the launch of the record that sees both is a full (shifted) one although the
    # DIFF vector is banded; the record that sees only the DIFF factor keeps its banded launch
    p = E.Plan(_two_edges("diff_shift", "diff"))
    for mode in C.MODES:
        for d in (0, 1):
            assert p.schedule_classes(d, mode) == {"diff": 3}
            info = p.diff_band_info(d, mode)
            assert 0 < info["band_launches"] < info["diff_launches"], info
    assert list(p.diff_bands()) == [1]                              # the DIFF factor's entry; the DIFF_SHIFT factor's reports -1
    for other in ("dense", "potts", "shared"):
        for L in (16, 40):
            cl = E.Plan(_two_edges("diff_shift", other, L)).schedule_classes(0, M.REPAM_UNIFORM)
            assert cl.pop("diff") == 1 and cl.pop("generic") in (1, 2) and sum(cl.values()) <= 1, (other, L, cl)
    # updated pairwise factors (`right` / `full` schedules) go to the generic classes
    for sched in C.UPDATED_SCHEDS:
        for L in (8, 40):
            cl = E.Plan(C.rules_grid(6, 5, L, sched=sched)).schedule_classes(0, M.REPAM_UNIFORM)
            assert cl and set(cl) <= GENERIC | ({"diff"} if sched == M.SCHED_FULL else set()), cl
            assert set(cl) & GENERIC
    # more labels than the class holds
    assert set(E.Plan(C.shift_grid(3, 2, 513, lengths=(5,))).schedule_classes(0, M.REPAM_ANISOTROPIC)) <= GENERIC


def test_plan_structure_and_bytes():
    """structure equals the expansion's; a receive accounts 16 bytes of constants where a plain DIFF receive accounts 8"""
    a, b = C.degenerate_pair()
    pa, pb, px = E.Plan(a), E.Plan(b), E.Plan(b.expand_diff())
    for d in (0, 1):
        assert np.array_equal(pb.order(d), px.order(d)) and np.array_equal(pb.update_order(d), px.update_order(d))
        for mode in C.MODES:
            assert np.array_equal(pb.update_levels(d, mode), px.update_levels(d, mode))
            ia, ib = pa.schedule_info(d, mode), pb.schedule_info(d, mode)
            for k in ("n_levels", "n_launches", "n_receives", "n_sends"):
                assert ia[k] == ib[k] == px.schedule_info(d, mode)[k]
            assert ib["algorithmic_bytes"] - ia["algorithmic_bytes"] == 8 * ia["n_receives"], (ia, ib)


def test_plans_without_the_kind_are_untouched():
    import diff_tables_cases as D
    V = np.stack([M.truncated_linear(40, 40, 0.2, 0.6), M.truncated_linear(40, 40, 0.3, 0.9)])
    p = E.Plan(S.grid_model(7, 6, 40, pairwise="diff", order="colour_major", seed=3, diff_tables=V))
    for mode in C.MODES:
        for d in (0, 1):
            assert p.schedule_classes(d, mode) == {"diff": 42}
            info = p.diff_band_info(d, mode)
            assert info["band_launches"] == info["diff_launches"] > 0 and info["band_receives"] == info["diff_receives"] > 0, info
    assert p.diff_bands() == {t: M.diff_band(v) + (True,) for t, v in enumerate(V)}
    q = E.Plan(D.label_grid(40, "colour_major"))                    # random vectors: the full kernel
    assert q.diff_band_info(0, M.REPAM_ANISOTROPIC)["band_launches"] == 0 and q.schedule_classes(0, M.REPAM_UNIFORM) == {"diff": 42}
    assert E.Plan(S.grid_model(4, 4, 8)).schedule_classes(0, M.REPAM_ANISOTROPIC) == {"dense8": 16}
    assert E.Plan(S.grid_model(4, 4, 8, pairwise="shared")).schedule_classes(0, M.REPAM_ANISOTROPIC) == {"shared8": 16}


def test_hosts_that_refuse_diff_refuse_the_kind_with_the_same_sentence(tmp_path):
    m, plain = C.shift_grid(3, 2, 5, lengths=(4,)), S.grid_model(3, 2, 5, pairwise="diff")
    msgs = []
    for model in (m, plain):
        with pytest.raises(ValueError) as ei:
            model.dump(str(tmp_path / "m.bin"))
        msgs.append(str(ei.value))
        with pytest.raises(ValueError) as ei:
            M.refuse_shared(model, "the multi-GPU hosts")
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[2] and msgs[1] == msgs[3]


def test_lp_mirror():
    from lp_mp_amd import lp as LPM
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.diff_shift_pairwise_factor, 1)
    Q = LPM.FactorContainer(LPM.PairwiseSimplexFactor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    for cont in (P, Q):
        lp = LPM.LP(LPM.FMC("SRMP", [U, cont], [ML, MR]))
        Dc, z = M.truncated_linear_compact(1.0, 2.0)
        t = lp.add_diff_table(Dc)
        u1, u2 = lp.add_factor(U, [0.0, 1.0, 2.0]), lp.add_factor(U, [1.0, 0.0, 3.0])
        p = lp.add_factor(P, 3, 3, t, 1.5, z + 4) if cont is P else lp.add_factor(Q, LPM.diff_shift_pairwise_factor(3, 3, t, 1.5, z + 4))
        lp.add_message(ML, u1, p); lp.add_message(MR, u2, p)
        f = lp.GetFactor(p)
        assert f.cost(0, 2) == 1.5 * 2.0 and f.cost(2, 0) == 1.5 * 2.0 and f.cost(0, 4 - 4) == 1.5 * 2.0
        m = lp.flat_model()
        assert list(m.f_kind) == [0, 0, M.F_PAIRWISE_DIFF_SHIFT] and list(m.const_data) == [1.5, float(z + 4)]
        got = m.expand_diff().const_data.reshape(3, 3)
        assert np.array_equal(got, np.array([[f.cost(a, b) for b in range(3)] for a in range(3)]))
        lp.set_factor_cost(p, 3, 3, t, 0.5, -1)
        assert list(lp.flat_model().const_data) == [0.5, -1.0]
        with pytest.raises(RuntimeError):
            lp.set_factor_cost(p, 3, 4, t, 0.5, -1)
    with pytest.raises(RuntimeError):
        LPM.diff_shift_pairwise_factor(3, 3, 0, 1.0, 0.5)


def test_the_oracle_runs_every_expansion_the_gpu_tests_use():
    n = 0
    for name, m in C.gpu_expansion_cases():
        x = C.expand(m)
        assert not x.has_diff and not x.has_shared, name
        E.Plan(m)                                                    # the plan takes the model (before the kind: "unknown kind")
        o = Oracle(x)
        o.set_reparametrization(M.REPAM_ANISOTROPIC)
        o.ComputePass(1)
        lb = o.LowerBound()
        assert np.isfinite(lb), (name, lb)
        assert not np.any(np.isnan(o.duals())), name
        n += 1
    assert n > 150
