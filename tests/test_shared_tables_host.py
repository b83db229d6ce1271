"""Shared pairwise tables (F_PAIRWISE_SHARED) on the host: model format, expansion, plan, kernel classes, byte accounting,
validation, the UAI reader — no GPU.  A SHARED factor is bit for bit a DENSE factor whose table is np.float64(scale) * V, so
every structural answer of the plan must equal that of ``expand_shared()``."""
import json
import os
import pickle

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import shared_tables_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shared_tables_parent_plans.json")


def test_builder_and_expansion():
    rng = np.random.default_rng(1)
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = b.add_vector_factors(0, rng.uniform(0, 1, (4, 3)))
    V = [rng.uniform(0, 1, (3, 3)), rng.uniform(0, 1, (3, 3))]
    t = [b.add_shared_table(v) for v in V]
    assert t == [0, 1]
    d = b.add_dense_pairwise(1, rng.uniform(0, 1, (1, 3, 3)))
    scales = np.array([0.5, 1.75, -2.0])
    p = b.add_shared_pairwise(1, [t[1], t[0], t[1]], scales)
    assert list(p) == [5, 6, 7] and list(d) == [4]
    for k, f in enumerate([d[0], p[0], p[1]]):
        b.add_messages(0, u[k], f); b.add_messages(1, u[k + 1], f)
    b.add_relations([u[0], d[0]], [d[0], u[1]])
    m = b.finish()
    assert m.has_shared and m.n_shared_tables == 2
    assert list(m.f_kind) == [0, 0, 0, 0, M.F_PAIRWISE_DENSE] + [M.F_PAIRWISE_SHARED] * 3
    assert list(m.f_table) == [-1] * 5 + [1, 0, 1]
    assert list(m.const_sizes()) == [0, 0, 0, 0, 9, 1, 1, 1] and list(m.dual_sizes()) == [3, 3, 3, 3, 6, 6, 6, 6]
    x = m.expand_shared()
    assert not x.has_shared and x.n_shared_tables == 0 and x.f_table is None
    assert list(x.f_kind) == [0, 0, 0, 0] + [M.F_PAIRWISE_DENSE] * 4
    co = x.const_offsets()
    assert np.array_equal(x.const_data[co[4]:co[5]], m.const_data[:9])
    for k, (ti, s) in enumerate(zip([1, 0, 1], scales)):
        assert np.array_equal(x.const_data[co[5 + k]:co[6 + k]].reshape(3, 3), np.float64(s) * V[ti])
    assert np.array_equal(m.dual_offsets(), x.dual_offsets()) and np.array_equal(m.dual_sizes(), x.dual_sizes())
    assert np.array_equal(m.dual_data, x.dual_data)
    for name in ("m_type", "m_left", "m_right", "rel_fwd", "rel_bwd", "f_type", "f_dim0", "f_dim1"):
        assert np.array_equal(getattr(m, name), getattr(x, name)), name
    m2 = pickle.loads(pickle.dumps(m))
    assert np.array_equal(m2.sh_data, m.sh_data) and np.array_equal(m2.f_table, m.f_table)
    # a model without the kind expands to itself
    g = S.grid_model(4, 4, 3)
    assert np.array_equal(g.expand_shared().const_data, g.const_data)
    with pytest.raises(ValueError):
        b.add_shared_pairwise(1, [7], [1.0])


@pytest.mark.parametrize("order", C.ORDERS)
def test_plan_structure_equals_the_expansions(order):
    m = S.grid_model(9, 7, 8, pairwise="shared", order=order, seed=3, n_tables=3)
    x = m.expand_shared()
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


@pytest.mark.parametrize("L", C.FAST_LABELS)
@pytest.mark.parametrize("order", C.ORDERS)
@pytest.mark.parametrize("n_tables", [1, 2, 4])
def test_fast_class_takes_every_update_of_a_shared_grid(L, order, n_tables):
    """the condition the GPU tests of the fast class assert first: the plan names ONLY the shared class of the padded width"""
    m = S.grid_model(13, 11, L, pairwise="shared", order=order, seed=L, n_tables=n_tables)
    p = E.Plan(m)
    n_upd = 13 * 11
    for mode in C.MODES:
        for d in (0, 1):
            assert p.schedule_classes(d, mode) == {"shared%d" % C.width_of(L): n_upd}, (L, order, mode, d)


def test_fast_class_conditions_of_the_other_gpu_inputs():
    for kind in C.SCALE_KINDS:
        m = C.shared_grid(13, 11, 32, order="colour_major", seed=9, scales=kind)
        assert set(E.Plan(m).schedule_classes(0, M.REPAM_ANISOTROPIC)) == {"shared32"}
    assert set(E.Plan(C.rect_chain()).schedule_classes(0, M.REPAM_UNIFORM)) == {"shared16"}
    m = S.grid_model(64, 64, 32, pairwise="shared", order="colour_major")
    assert E.Plan(m).schedule_classes(0, M.REPAM_ANISOTROPIC) == {"shared32": 64 * 64}


def test_fallback_classes():
    generic = {"generic", "small"}
    # more than 32 labels
    assert set(E.Plan(S.grid_model(5, 6, 40, pairwise="shared")).schedule_classes(0, M.REPAM_ANISOTROPIC)) <= generic
    # updated SHARED pairwise factors (`right` / `full` schedules)
    for sched in (M.SCHED_RIGHT, M.SCHED_FULL):
        cl = E.Plan(C.rules_grid(6, 5, 8, sched=sched)).schedule_classes(0, M.REPAM_UNIFORM)
        assert cl and set(cl) <= generic | ({"shared8"} if sched == M.SCHED_FULL else set()), cl
        assert "generic" in cl or "small" in cl
    # a mixed neighbourhood: SHARED beside DENSE peers
    rng = np.random.default_rng(2)
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = b.add_vector_factors(0, rng.uniform(0, 1, (3, 16)))
    t = b.add_shared_table(rng.uniform(0, 1, (16, 16)))
    p0 = b.add_shared_pairwise(1, [t], [1.5])[0]
    p1 = b.add_dense_pairwise(1, rng.uniform(0, 1, (1, 16, 16)))[0]
    b.add_messages(0, u[0], p0); b.add_messages(1, u[1], p0); b.add_messages(0, u[1], p1); b.add_messages(1, u[2], p1)
    b.add_relations([u[0], p0, u[1], p1], [p0, u[1], p1, u[2]])
    cl = E.Plan(b.finish()).schedule_classes(0, M.REPAM_UNIFORM)
    # u0 sees only the SHARED factor, u2 only the DENSE one, u1 both
    # (the dense one on the run-time-dims form: its table starts at an odd offset behind the SHARED factor's one double)
    assert cl == {"generic": 1, "shared16": 1, "dense_v16": 1}, cl
    # more distinct tables than a launch's LDS budget (4): the level is split by table set into several launches of the class ...
    for nt in (5, 8):
        p = E.Plan(S.grid_model(20, 20, 32, pairwise="shared", order="colour_major", n_tables=nt))
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            assert p.schedule_classes(0, mode) == {"shared32": 400}
            assert p.schedule_info(0, mode)["n_launches"] > p.schedule_info(0, mode)["n_levels"]
    # ... and what no group of a level takes (at most 32 groups) runs on the generic class
    cl = E.Plan(S.grid_model(20, 20, 32, pairwise="shared", order="colour_major", n_tables=40)).schedule_classes(0, M.REPAM_UNIFORM)
    assert set(cl) == {"generic", "shared32"} and sum(cl.values()) == 400


@pytest.mark.parametrize("L", [4, 13, 32])
def test_algorithmic_bytes(L):
    m = S.grid_model(13, 11, L, pairwise="shared", order="colour_major", seed=1)
    p, q = E.Plan(m), E.Plan(m.expand_shared())
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        for d in (0, 1):
            a, b = p.schedule_info(d, mode), q.schedule_info(d, mode)
            assert a["n_receives"] == b["n_receives"] > 0
            assert a["algorithmic_bytes"] == b["algorithmic_bytes"] - a["n_receives"] * (8 * L * L - 8)
        a, b = p.pass_schedule_info(mode), q.pass_schedule_info(mode)
        assert a["algorithmic_bytes"] == b["algorithmic_bytes"] - a["n_receives"] * (8 * L * L - 8)


def _summary(m):
    p = E.Plan(m)
    out = {}
    for name, mode in (("anisotropic", M.REPAM_ANISOTROPIC), ("uniform", M.REPAM_UNIFORM)):
        out[name] = {"schedule_classes": [p.schedule_classes(d, mode) for d in (0, 1)],
                     "schedule_info": [p.schedule_info(d, mode) for d in (0, 1)],
                     "chain_info": [p.chain_info(d, mode) for d in (0, 1, -1)],
                     "pass_rotates": p.pass_rotates(mode)}
    return out


def test_plans_of_models_without_the_kind_are_the_parents():
    """recorded from the parent commit with this same function (tests/golden/shared_tables_parent_plans.json)"""
    golden = json.load(open(GOLDEN))
    models = {
        "grid_64_64_32_dense_colour_major": S.grid_model(64, 64, 32, order="colour_major", seed=3),
        "grid_64_64_32_dense_row_major": S.grid_model(64, 64, 32, seed=3),
        "grid_40_30_8_potts_colour_major": S.grid_model(40, 30, 8, pairwise="potts", order="colour_major", seed=5),
        "random_graph_300_900_13_dense": S.random_graph_model(300, 900, 13, seed=11),
    }
    assert set(models) == set(golden)
    for k, m in models.items():
        assert json.loads(json.dumps(_summary(m))) == golden[k], k


def test_validation():
    m = S.grid_model(4, 3, 5, pairwise="shared", n_tables=2)
    E.Plan(m)
    f = int(np.nonzero(m.f_kind == M.F_PAIRWISE_SHARED)[0][3])
    import dataclasses
    bad = dataclasses.replace(m, f_table=m.f_table.copy(), _keep=[])
    bad.f_table[f] = 2
    with pytest.raises(RuntimeError, match="factor %d" % f):
        E.Plan(bad)
    bad.f_table[f] = -1
    with pytest.raises(RuntimeError, match="factor %d" % f):
        E.Plan(bad)
    bad = dataclasses.replace(m, f_dim1=m.f_dim1.copy(), _keep=[])
    bad.f_dim1[f] = 4
    with pytest.raises(RuntimeError, match="factor %d" % f):
        E.Plan(bad)
    bad = dataclasses.replace(m, f_table=None, _keep=[])
    with pytest.raises(RuntimeError, match="factor %d" % int(np.nonzero(m.f_kind == M.F_PAIRWISE_SHARED)[0][0])):
        E.Plan(bad)
    bad = dataclasses.replace(m, sh_off=m.sh_off + 1, _keep=[])
    with pytest.raises(RuntimeError, match="shared table"):
        E.Plan(bad)
    bad = dataclasses.replace(m, sh_data=m.sh_data.copy(), _keep=[])
    bad.sh_data[30] = np.nan
    with pytest.raises(RuntimeError, match="shared table 1: NaN"):
        E.Plan(bad)


def test_dump_and_multi_gpu_hosts_refuse(tmp_path):
    m = S.grid_model(6, 6, 4, pairwise="shared", order="colour_major")
    with pytest.raises(ValueError, match="shared"):
        m.dump(str(tmp_path / "m.bin"))
    m.expand_shared().dump(str(tmp_path / "x.bin"))
    from lp_mp_amd import lockstep, multi_gpu, overlap
    part = np.zeros(m.n_factors, np.int64)
    with pytest.raises(ValueError, match="shared"):
        multi_gpu.partition_model(m, part, 2)
    with pytest.raises(ValueError, match="shared"):
        multi_gpu.graph_partition_model(m, 2)
    with pytest.raises(ValueError, match="shared"):
        lockstep.lockstep_model(m, part, 2, M.REPAM_ANISOTROPIC)
    with pytest.raises(ValueError, match="shared"):
        multi_gpu.strip_local_part(8, 8, 4, "shared", "colour_major", 0, 2, 1)
    with pytest.raises(ValueError, match="shared"):
        overlap.grid_pass_counts(8, 8, 4, "shared")


def test_synthetic_options_leave_existing_streams_alone():
    a = S.grid_model(5, 4, 3, seed=2)
    assert np.array_equal(a.const_data, S.u01(31 * 9, 2, 60))
    m = S.grid_model(5, 4, 3, pairwise="shared", seed=2, n_tables=2)
    assert np.array_equal(m.sh_data, S.u01(2 * 9, 2, 60))
    assert np.array_equal(m.const_data, 0.5 + 1.5 * S.u01(31, 2, 60 + 18)) and m.const_data.min() >= 0.5 and m.const_data.max() < 2.0
    sh = np.nonzero(m.f_kind == M.F_PAIRWISE_SHARED)[0]
    assert np.array_equal(m.f_table[sh], np.arange(31) % 2)
    r = S.random_graph_model(30, 60, 5, seed=3, pairwise="shared", n_tables=3)
    assert r.n_shared_tables == 3 and int((r.f_kind == M.F_PAIRWISE_SHARED).sum()) == 60
    E.Plan(r)


def test_uai_share_tables():
    from lp_mp_amd import uai
    a = uai.build_lp_from_uai(C.UAI_TEXT).flat_model()
    b = uai.build_lp_from_uai(C.UAI_TEXT, share_tables=True).flat_model()
    assert not a.has_shared and a.n_shared_tables == 0
    assert b.n_shared_tables == 2 and int((b.f_kind == M.F_PAIRWISE_SHARED).sum()) == 3
    x = b.expand_shared()
    for name in ("f_type", "f_kind", "f_flags", "f_dim0", "f_dim1", "const_data", "dual_data", "m_type", "m_left", "m_right", "rel_fwd", "rel_bwd"):
        assert np.array_equal(getattr(a, name), getattr(x, name)), name


def test_lp_mirror_shared_factor_op():
    from lp_mp_amd import lp as LPM
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.shared_pairwise_factor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    lp = LPM.LP(LPM.FMC("FMC", [U, P], [ML, MR]))
    t = lp.add_shared_table([[0.0, 1.0], [1.0, 0.0]])
    u0, u1 = lp.add_factor(U, [0.0, 1.0]), lp.add_factor(U, [2.0, 0.5])
    p = lp.add_factor(P, t, 3.0)
    lp.add_message(ML, u0, p); lp.add_message(MR, u1, p)
    assert lp.GetFactor(p).cost(0, 1) == 3.0 and lp.GetFactor(p).cost(1, 1) == 0.0 and (lp.GetFactor(p).dim1, lp.GetFactor(p).dim2) == (2, 2)
    m = lp.flat_model()
    assert list(m.f_kind) == [0, 0, M.F_PAIRWISE_SHARED] and m.const_data[0] == 3.0 and list(m.f_table) == [-1, -1, 0]
    with pytest.raises(RuntimeError):
        lp.add_factor(P, 5, 1.0)


def test_oracle_runs_every_expansion_of_the_gpu_tests():
    n = 0
    for name, m in C.gpu_expansion_cases():
        n += 1
        x = m.expand_shared()
        assert not x.has_shared
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            o = Oracle(x)
            o.set_reparametrization(mode)
            lb0 = o.LowerBound()
            o.ComputePass(2)
            lb = o.LowerBound()
            assert np.isfinite(lb0) and np.isfinite(lb) and lb >= lb0 - 1e-9 * max(1.0, abs(lb0)), (name, mode, lb0, lb)
            assert not np.any(np.isnan(o.duals())), name
    assert n >= 48 + C.N_FUZZ
