"""Difference-indexed pairwise factors (F_PAIRWISE_DIFF) on the host: model format, expansion, plan, the kernel class, byte
accounting, validation, the UAI reader — no GPU.  A DIFF factor is bit for bit a DENSE factor whose table is
np.float64(scale) * D[a - b + d1 - 1], so every structural answer of the plan must equal that of ``expand_diff()``."""
import dataclasses
import pickle

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import diff_tables_cases as C
import schedule_hazards as H

GENERIC = {"generic", "small"}


def _dense_table(D, d0, d1, scale):
    return np.array([[np.float64(scale) * D[a - b + d1 - 1] for b in range(d1)] for a in range(d0)])


def test_builder_and_expansion():
    rng = np.random.default_rng(1)
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = b.add_vector_factors(0, rng.uniform(0, 1, (4, 3)))
    D = [rng.uniform(0, 1, 5), rng.uniform(0, 1, 5)]
    t = [b.add_diff_table(v) for v in D]
    assert t == [0, 1]
    d = b.add_dense_pairwise(1, rng.uniform(0, 1, (1, 3, 3)))
    scales = np.array([0.5, 1.75, -2.0])
    p = b.add_diff_pairwise(1, 3, 3, [t[1], t[0], t[1]], scales)
    assert list(p) == [5, 6, 7] and list(d) == [4]
    for k, f in enumerate([d[0], p[0], p[1]]):
        b.add_messages(0, u[k], f); b.add_messages(1, u[k + 1], f)
    b.add_relations([u[0], d[0]], [d[0], u[1]])
    m = b.finish()
    assert m.has_diff and not m.has_shared and m.n_shared_tables == 2
    assert list(m.sh_dim0) == [1, 1] and list(m.sh_dim1) == [5, 5]
    assert list(m.f_kind) == [0, 0, 0, 0, M.F_PAIRWISE_DENSE] + [M.F_PAIRWISE_DIFF] * 3 and M.F_PAIRWISE_DIFF == 4
    assert list(m.f_table) == [-1] * 5 + [1, 0, 1]
    assert list(m.const_sizes()) == [0, 0, 0, 0, 9, 1, 1, 1] and list(m.dual_sizes()) == [3, 3, 3, 3, 6, 6, 6, 6]
    x = m.expand_diff()
    assert not x.has_diff and x.n_shared_tables == 0 and x.f_table is None
    assert list(x.f_kind) == [0, 0, 0, 0] + [M.F_PAIRWISE_DENSE] * 4
    co = x.const_offsets()
    assert np.array_equal(x.const_data[co[4]:co[5]], m.const_data[:9])
    for k, (ti, s) in enumerate(zip([1, 0, 1], scales)):
        got = x.const_data[co[5 + k]:co[6 + k]].reshape(3, 3)
        assert got.tobytes() == _dense_table(D[ti], 3, 3, s).tobytes()
    assert np.array_equal(m.dual_offsets(), x.dual_offsets()) and np.array_equal(m.dual_data, x.dual_data)
    for name in ("m_type", "m_left", "m_right", "rel_fwd", "rel_bwd", "f_type", "f_dim0", "f_dim1"):
        assert np.array_equal(getattr(m, name), getattr(x, name)), name
    m2 = pickle.loads(pickle.dumps(m))
    assert np.array_equal(m2.sh_data, m.sh_data) and np.array_equal(m2.f_table, m.f_table)
    # models without the kind expand to themselves; expand_shared leaves DIFF factors and their pool alone
    g = S.grid_model(4, 4, 3)
    assert np.array_equal(g.expand_diff().const_data, g.const_data)
    y = m.expand_shared()
    assert y.has_diff and np.array_equal(y.f_table, m.f_table) and np.array_equal(y.const_data, m.const_data)
    with pytest.raises(ValueError):
        b.add_diff_pairwise(1, 3, 3, [7], [1.0])
    with pytest.raises(ValueError):
        b.add_diff_pairwise(1, 3, 4, [0], [1.0])       # 3 x 4 needs 6 entries


def test_rectangular_expansion_and_a_model_with_both_pooled_kinds():
    rng = np.random.default_rng(2)
    m = C.rect_chain(n=4, seed=2, dims=(3, 7))
    x = m.expand_diff()
    co, mo = x.const_offsets(), m.const_offsets()
    for f in np.nonzero(m.f_kind == M.F_PAIRWISE_DIFF)[0]:
        d0, d1 = int(m.f_dim0[f]), int(m.f_dim1[f])
        assert {d0, d1} == {3, 7}
        D = m.shared_table(int(m.f_table[f])).reshape(-1)
        assert D.shape[0] == 9
        assert x.const_data[co[f]:co[f + 1]].tobytes() == _dense_table(D, d0, d1, m.const_data[mo[f]]).tobytes()
    g = C.mixed_graph(rng, n=20)
    assert g.has_diff and g.has_shared
    a, b = g.expand_diff(), g.expand_shared()
    assert a.has_shared and not a.has_diff and b.has_diff and not b.has_shared
    for full in (a.expand_shared(), b.expand_diff(), C.expand(g)):
        assert not full.has_diff and not full.has_shared and full.f_table is None and full.n_shared_tables == 0
    assert np.array_equal(a.expand_shared().const_data, b.expand_diff().const_data)


def test_potential_constructors():
    D = M.truncated_linear(4, 6, 0.3, 1.0)
    assert D.shape == (9,) and D.tobytes() == np.array([min(np.float64(0.3) * abs(k - 5), 1.0) for k in range(9)]).tobytes()
    Q = M.truncated_quadratic(6, 4, 0.3, 2.0)
    assert Q.shape == (9,) and Q.tobytes() == np.array([min(np.float64(0.3) * np.float64((k - 3) * (k - 3)), 2.0) for k in range(9)]).tobytes()
    b = M.ModelBuilder(2, S.mrf_mtypes())
    b.add_vector_factors(0, np.zeros((2, 4)))
    b.add_diff_pairwise(1, 4, 6, [b.add_diff_table(D)], [2.0])
    x = b.finish().expand_diff()
    want = np.array([[2.0 * min(np.float64(0.3) * abs(a - c), 1.0) for c in range(6)] for a in range(4)])
    assert x.const_data.tobytes() == want.tobytes()


@pytest.mark.parametrize("order", C.ORDERS)
def test_plan_structure_equals_the_expansions(order):
    m = S.grid_model(9, 7, 40, pairwise="diff", order=order, seed=3, n_tables=3)
    x = m.expand_diff()
    p, q = E.Plan(m), E.Plan(x)
    for d in (0, 1):
        assert np.array_equal(p.order(d), q.order(d)) and np.array_equal(p.update_order(d), q.update_order(d))
        for mode in C.MODES:
            for a, b in zip(p.omega(d, mode) + p.mask(d, mode), q.omega(d, mode) + q.mask(d, mode)):
                assert np.array_equal(a, b)
            assert np.array_equal(p.update_levels(d, mode), q.update_levels(d, mode))
            ip, iq = p.schedule_info(d, mode), q.schedule_info(d, mode)
            for k in ("n_levels", "n_launches", "n_receives", "n_sends"):
                assert ip[k] == iq[k], (k, ip, iq)
    for a, b in zip(p.msg_lists(m.n_messages), q.msg_lists(x.n_messages)):
        assert np.array_equal(a, b)
    (ra, ka), (rb, kb) = p.suggest_order(0), q.suggest_order(0)
    assert ka == kb and np.array_equal(ra, rb)
    for mode in C.MODES:
        assert p.pass_rotates(mode) == q.pass_rotates(mode)


@pytest.mark.parametrize("L", C.CLASS_LABELS)
@pytest.mark.parametrize("order", C.ORDERS)
def test_the_class_takes_every_update_of_a_diff_grid(L, order):
    """the condition the GPU tests assert first: the plan names ONLY the class, at every label count"""
    m = S.grid_model(7, 6, L, pairwise="diff", order=order, seed=L)
    p = E.Plan(m)
    for mode in C.MODES:
        for d in (0, 1):
            assert p.schedule_classes(d, mode) == {"diff": 42}, (L, order, mode, d)


def test_class_conditions_of_the_other_gpu_inputs():
    for kw in C.RECT_CHAINS:
        m = C.rect_chain(**kw)
        n_upd = int((m.f_kind == M.F_VECTOR).sum())
        for mode in C.MODES:
            assert E.Plan(m).schedule_classes(0, mode) == {"diff": n_upd}
    for nt in C.VECTOR_COUNTS:                      # no table budget: any number of vectors in a level
        m = C.vectors_grid(nt)
        assert m.n_shared_tables == nt
        p = E.Plan(m)
        assert p.schedule_classes(0, M.REPAM_UNIFORM) == {"diff": 12 * 11}
        assert p.schedule_info(0, M.REPAM_UNIFORM)["n_launches"] == p.schedule_info(0, M.REPAM_UNIFORM)["n_levels"]
    for kind in C.SCALE_KINDS:
        assert set(E.Plan(C.scale_grid(40, "colour_major", kind)).schedule_classes(0, M.REPAM_ANISOTROPIC)) == {"diff"}


def test_fallback_classes():
    # updated DIFF pairwise factors (`right` / `full` schedules)
    for sched in (M.SCHED_RIGHT, M.SCHED_FULL):
        for L in (8, 40):
            cl = E.Plan(C.rules_grid(6, 5, L, sched=sched)).schedule_classes(0, M.REPAM_UNIFORM)
            assert cl and set(cl) <= GENERIC | ({"diff"} if sched == M.SCHED_FULL else set()), cl
            assert set(cl) & GENERIC
    # mixed neighbourhoods: DIFF beside a DENSE, a POTTS and a SHARED peer
    rng = np.random.default_rng(2)
    for other in ("dense", "potts", "shared"):
        for L in (16, 40):
            b = M.ModelBuilder(2, S.mrf_mtypes())
            u = b.add_vector_factors(0, rng.uniform(0, 1, (3, L)))
            p0 = b.add_diff_pairwise(1, L, L, [b.add_diff_table(rng.uniform(0, 1, 2 * L - 1))], [1.5])[0]
            if other == "dense":
                p1 = b.add_dense_pairwise(1, rng.uniform(0, 1, (1, L, L)))[0]
            elif other == "potts":
                p1 = b.add_potts_pairwise(1, L, [0.7])[0]
            else:
                p1 = b.add_shared_pairwise(1, [b.add_shared_table(rng.uniform(0, 1, (L, L)))], [0.7])[0]
            b.add_messages(0, u[0], p0); b.add_messages(1, u[1], p0); b.add_messages(0, u[1], p1); b.add_messages(1, u[2], p1)
            b.add_relations([u[0], p0, u[1], p1], [p0, u[1], p1, u[2]])
            cl = E.Plan(b.finish()).schedule_classes(0, M.REPAM_UNIFORM)
            # u0 sees only the DIFF factor, u2 only the other one (a class of its kind, or generic for SHARED beyond 32 labels), u1 both
            assert cl.pop("diff") == 1 and cl.pop("generic") in (1, 2) and sum(cl.values()) <= 1, (other, L, cl)
            assert not set(cl) & {"diff"} and all(k.startswith(other) or k == "dense_big" for k in cl), (other, L, cl)
    # more labels than the class holds
    assert set(E.Plan(S.grid_model(3, 2, 513, pairwise="diff")).schedule_classes(0, M.REPAM_ANISOTROPIC)) <= GENERIC
    # two DIFF factors between the same two variables are NOT duplicate vectors; two messages of one factor to one unary are
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = b.add_vector_factors(0, rng.uniform(0, 1, (2, 40)))
    t = b.add_diff_table(rng.uniform(0, 1, 79))
    p = b.add_diff_pairwise(1, 40, 40, [t, t], [1.0, 2.0])
    for f in p:
        b.add_messages(0, u[0], f); b.add_messages(1, u[1], f)
        b.add_relations([u[0], f], [f, u[1]])
    assert E.Plan(b.finish()).schedule_classes(0, M.REPAM_UNIFORM) == {"diff": 2}
    # duplicate vectors: the same message twice between one unary and one DIFF factor.  sweep_diff_kernel requests m_o and m_s of
    # a receive together and is not written for two ops on one vector, so the record must NOT be of class diff: u0 (two
    # receives from / two sends into m1 of the factor) goes to the op-by-op generic kernels, u1 (one message) stays diff
    for L, want in ((8, "small"), (40, "generic")):
        b = M.ModelBuilder(2, S.mrf_mtypes())
        u = b.add_vector_factors(0, rng.uniform(0, 1, (2, L)))
        f = b.add_diff_pairwise(1, L, L, [b.add_diff_table(rng.uniform(0, 1, 2 * L - 1))], [1.5])[0]
        b.add_messages(0, u[0], f); b.add_messages(0, u[0], f); b.add_messages(1, u[1], f)
        b.add_relations([u[0], f], [f, u[1]])
        m = b.finish()
        for d in (0, 1):
            for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
                assert E.Plan(m).schedule_classes(d, mode) == {want: 1, "diff": 1}, (L, d, mode)


@pytest.fixture(scope="module")
def probe_lib(tmp_path_factory):
    return H.build_probe(tmp_path_factory.mktemp("schedule_probe"))


def test_forced_generic_plan_has_no_diff_class(probe_lib):
    """the adaptive rule plans with Plan::force_generic (engine.cpp): every record of a DIFF grid then runs on the generic
    kernels, which read the kind through pw_cost, and none on class diff"""
    for L in (8, 40):
        m = S.grid_model(5, 4, L, pairwise="diff", order="colour_major", seed=3)
        p = E.Plan(m)
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            for d in (0, 1):
                seg = (p.update_order(d),) + p.omega(d, mode) + p.mask(d, mode)
                got = {}
                for forced in (False, True):
                    sch = H.Probe(probe_lib, m, force_generic=forced).plan([seg], fuse=False)
                    got[forced] = {E.KCLASS_NAMES[c] for c in sch["rec_class"]}
                    assert len(sch["rec_class"]) == 20
                assert got[False] == {"diff"} and got[True] and got[True] <= GENERIC, (L, mode, d, got)


@pytest.mark.parametrize("L", [4, 13, 40, 130])
def test_algorithmic_bytes(L):
    m = S.grid_model(7, 6, L, pairwise="diff", order="colour_major", seed=1)
    p, q = E.Plan(m), E.Plan(m.expand_diff())
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        for d in (0, 1):
            a, b = p.schedule_info(d, mode), q.schedule_info(d, mode)
            assert a["n_receives"] == b["n_receives"] > 0
            assert a["algorithmic_bytes"] == b["algorithmic_bytes"] - a["n_receives"] * (8 * L * L - 8)
        a, b = p.pass_schedule_info(mode), q.pass_schedule_info(mode)
        assert a["algorithmic_bytes"] == b["algorithmic_bytes"] - a["n_receives"] * (8 * L * L - 8)


def test_validation():
    m = S.grid_model(4, 3, 5, pairwise="diff", n_tables=2)
    E.Plan(m)
    diff = np.nonzero(m.f_kind == M.F_PAIRWISE_DIFF)[0]
    f = int(diff[3])
    # a vector of the wrong length
    bad = dataclasses.replace(m, f_dim1=m.f_dim1.copy(), _keep=[])
    bad.f_dim1[f] = 4
    with pytest.raises(RuntimeError, match="factor %d" % f):
        E.Plan(bad)
    # a table that is not a vector (sh_dim0 != 1): 3 x 3 = 9 entries, as many as the vector
    bad = dataclasses.replace(m, sh_dim0=np.array([1, 3], np.int32), sh_dim1=np.array([9, 3], np.int32), _keep=[])
    with pytest.raises(RuntimeError, match="factor %d" % int(diff[1])):
        E.Plan(bad)
    # index out of range
    bad = dataclasses.replace(m, f_table=m.f_table.copy(), _keep=[])
    for t in (2, -1):
        bad.f_table[f] = t
        with pytest.raises(RuntimeError, match="factor %d" % f):
            E.Plan(bad)
    # no f_table
    bad = dataclasses.replace(m, f_table=None, _keep=[])
    with pytest.raises(RuntimeError, match="factor %d" % int(diff[0])):
        E.Plan(bad)
    # NaN in the pool
    bad = dataclasses.replace(m, sh_data=m.sh_data.copy(), _keep=[])
    bad.sh_data[12] = np.nan
    with pytest.raises(RuntimeError, match="shared table 1: NaN"):
        E.Plan(bad)
    # a kind beyond DIFF is unknown
    bad = dataclasses.replace(m, f_kind=m.f_kind.copy(), _keep=[])
    bad.f_kind[f] = 5
    with pytest.raises(RuntimeError, match="factor %d: unknown kind" % f):
        E.Plan(bad)


def test_dump_and_multi_gpu_hosts_refuse(tmp_path):
    m = S.grid_model(6, 6, 4, pairwise="diff", order="colour_major")
    with pytest.raises(ValueError, match="difference-indexed"):
        m.dump(str(tmp_path / "m.bin"))
    m.expand_diff().dump(str(tmp_path / "x.bin"))
    from lp_mp_amd import lockstep, multi_gpu, overlap
    part = np.zeros(m.n_factors, np.int64)
    with pytest.raises(ValueError, match="difference-indexed"):
        multi_gpu.partition_model(m, part, 2)
    with pytest.raises(ValueError, match="difference-indexed"):
        multi_gpu.graph_partition_model(m, 2)
    with pytest.raises(ValueError, match="difference-indexed"):
        lockstep.lockstep_model(m, part, 2, M.REPAM_ANISOTROPIC)
    with pytest.raises(ValueError, match="difference-indexed"):
        multi_gpu.strip_local_part(8, 8, 4, "diff", "colour_major", 0, 2, 1)
    with pytest.raises(ValueError, match="difference-indexed"):
        overlap.grid_pass_counts(8, 8, 4, "diff")


def test_synthetic_streams():
    m = S.grid_model(5, 4, 3, pairwise="diff", seed=2, n_tables=2)
    assert np.array_equal(m.sh_data, S.u01(2 * 5, 2, 60))
    assert np.array_equal(m.const_data, 0.5 + 1.5 * S.u01(31, 2, 60 + 10))
    df = np.nonzero(m.f_kind == M.F_PAIRWISE_DIFF)[0]
    assert np.array_equal(m.f_table[df], np.arange(31) % 2)
    r = S.random_graph_model(30, 60, 5, seed=3, pairwise="diff", n_tables=3)
    assert r.n_shared_tables == 3 and int((r.f_kind == M.F_PAIRWISE_DIFF).sum()) == 60
    E.Plan(r)
    # the other options keep their streams
    assert np.array_equal(S.grid_model(5, 4, 3, seed=2).const_data, S.u01(31 * 9, 2, 60))
    assert np.array_equal(S.grid_model(5, 4, 3, pairwise="shared", seed=2, n_tables=2).sh_data, S.u01(2 * 9, 2, 60))


def test_uai_diff_tables():
    from lp_mp_amd import uai
    a = uai.build_lp_from_uai(C.UAI_TEXT).flat_model()
    b = uai.build_lp_from_uai(C.UAI_TEXT, diff_tables=True).flat_model()
    assert not a.has_diff and a.n_shared_tables == 0
    # 0-1 and 1-2 share one vector, 2-3 (3 x 2 labels) has its own, 0-2 is no function of a - b and stays dense
    assert list(b.f_kind[4:]) == [M.F_PAIRWISE_DIFF] * 3 + [M.F_PAIRWISE_DENSE]
    assert b.n_shared_tables == 2 and list(b.f_table[4:]) == [0, 0, 1, -1] and list(b.sh_dim1) == [5, 4]
    x = b.expand_diff()
    for name in ("f_type", "f_kind", "f_flags", "f_dim0", "f_dim1", "dual_data", "m_type", "m_left", "m_right", "rel_fwd", "rel_bwd"):
        assert np.array_equal(getattr(a, name), getattr(x, name)), name
    assert a.const_data.tobytes() == x.const_data.tobytes()
    # with both options a table that is no difference vector is pooled as a shared table
    c = uai.build_lp_from_uai(C.UAI_TEXT, diff_tables=True, share_tables=True).flat_model()
    assert list(c.f_kind[4:]) == [M.F_PAIRWISE_DIFF] * 3 + [M.F_PAIRWISE_SHARED]
    assert a.const_data.tobytes() == C.expand(c).const_data.tobytes()
    # colour-major orientation transposes tables: the difference vector is then read the other way round
    d = uai.build_lp_from_uai(C.UAI_TEXT, diff_tables=True, order="colour_major").flat_model()
    e = uai.build_lp_from_uai(C.UAI_TEXT, order="colour_major").flat_model()
    assert d.has_diff and d.expand_diff().const_data.tobytes() == e.const_data.tobytes()


def test_lp_mirror_diff_factor_op():
    from lp_mp_amd import lp as LPM
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.diff_pairwise_factor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    lp = LPM.LP(LPM.FMC("FMC", [U, P], [ML, MR]))
    D = [2.0, 1.0, 0.0, 0.5]                               # 2 x 3: cost(a, b) = D[a - b + 2]
    t = lp.add_diff_table(D)
    u0, u1 = lp.add_factor(U, [0.0, 1.0]), lp.add_factor(U, [2.0, 0.5, 0.1])
    p = lp.add_factor(P, t, 2, 3, 3.0)
    lp.add_message(ML, u0, p); lp.add_message(MR, u1, p)
    g = lp.GetFactor(p)
    assert g.cost(0, 0) == 0.0 and g.cost(0, 2) == 6.0 and g.cost(1, 0) == 1.5 and (g.dim1, g.dim2) == (2, 3)
    m = lp.flat_model()
    # the same FlatModel as the builder's
    b = M.ModelBuilder(2, m.mtypes, [1, 0])
    b.add_diff_table(D)
    b.add_vector_factors(0, [[0.0, 1.0]]); b.add_vector_factors(0, [[2.0, 0.5, 0.1]])
    b.add_diff_pairwise(1, 2, 3, [0], [3.0])
    b.add_messages(0, 0, 2); b.add_messages(1, 1, 2)
    w = b.finish()
    for name in ("f_type", "f_kind", "f_flags", "f_dim0", "f_dim1", "const_data", "dual_data", "m_type", "m_left", "m_right", "f_table",
                 "sh_off", "sh_dim0", "sh_dim1", "sh_data"):
        assert np.array_equal(getattr(m, name), getattr(w, name)), name
    with pytest.raises(RuntimeError):
        lp.add_factor(P, 5, 2, 3, 1.0)
    with pytest.raises(RuntimeError):
        lp.add_factor(P, t, 3, 3, 1.0)                    # 3 x 3 needs 5 entries


def test_oracle_runs_every_expansion_of_the_gpu_tests():
    n = 0
    for name, m in C.gpu_expansion_cases():
        n += 1
        x = C.expand(m)
        assert not x.has_diff and not x.has_shared, name
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            o = Oracle(x)
            o.set_reparametrization(mode)
            lb0 = o.LowerBound()
            o.ComputePass(2)
            lb = o.LowerBound()
            assert np.isfinite(lb0) and np.isfinite(lb) and lb >= lb0 - 1e-9 * max(1.0, abs(lb0)), (name, mode, lb0, lb)
            assert not np.any(np.isnan(o.duals())), name
    assert n == 89 + C.N_FUZZ
