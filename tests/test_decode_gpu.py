"""lpmp_decode_primal on the device against the numpy statement of the rule (tests/decode_cases.py).

Procedure: upload, anisotropic weights, 3 passes, download the duals, decode; ``download_primal`` — the unary labels and both slots
of every pairwise factor — must be ``np.array_equal`` to ``decode_reference`` on those downloaded duals, in both directions and with
0, 1 and 3 refinement sweeps.  The shapes are the smallest at which the kernel takes another path: label counts at the edges of the
lane groups (4 / 8 / 16 / 32 lanes), of the 64-lane stride and beyond two strides; rectangular tables with the unary on either side;
every pairwise kind and storage; hubs, isolated unaries, duplicate edges, +inf entries and exact ties."""
import dataclasses

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import lp as LPM
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

import decode_cases as C
import recost_cases as RC

pytestmark = pytest.mark.gpu

ANISO = M.REPAM_ANISOTROPIC
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -2, -4

# name -> (model, upload keywords)
CASES = {
    "labels1": (lambda: C.labels_case(1), {}),
    "labels2": (lambda: C.labels_case(2), {}),
    "labels13": (lambda: C.labels_case(13), {}),
    "labels32": (lambda: C.labels_case(32), {}),
    "labels33": (lambda: C.labels_case(33), {}),
    "labels64": (lambda: C.labels_case(64), {}),
    "labels65": (lambda: C.labels_case(65), {}),
    "labels130": (lambda: C.labels_case(130), {}),
    "rect5x9": (lambda: C.rect_case(5, 9), {}),
    "rect40x33": (lambda: C.rect_case(40, 33), {}),
    "dense_f32": (lambda: C.f32_case(), {"table_precision": "f32"}),
    "potts13": (lambda: C.labels_case(13, "potts"), {}),
    "potts65": (lambda: C.labels_case(65, "potts"), {}),
    "shared13": (lambda: C.labels_case(13, "shared"), {}),
    "shared65": (lambda: C.labels_case(65, "shared"), {}),
    "diff_full": (lambda: C.diff_case(False), {}),
    "diff_banded": (lambda: C.diff_case(True), {}),
    "diff130": (lambda: C.labels_case(130, "diff"), {}),
    "mixed": (lambda: C.mixed_case(), {}),
    "rows_layout": (lambda: C.labels_case(13), {"rows_layout": True}),
    "rows_layout_grid": (lambda: C.grid(9, 7, 8, "colour_major"), {"rows_layout": True}),
    "star70": (lambda: C.star(), {}),
    "duplicate_edges": (lambda: C.duplicate_edges(), {}),
    "inf_tables": (lambda: C.inf_tables_case(), {}),
    "ties_dense": (lambda: C.ties_case("dense"), {}),
    "ties_potts": (lambda: C.ties_case("potts"), {}),
    "ties_shared": (lambda: C.ties_case("shared"), {}),
    "ties_diff": (lambda: C.ties_case("diff"), {}),
    "grid_row_major": (lambda: C.grid(9, 7, 8, "row_major"), {}),
    "grid_colour_major": (lambda: C.grid(9, 7, 8, "colour_major"), {}),
    "grid_colour_major_potts": (lambda: C.grid(9, 7, 8, "colour_major", "potts"), {}),
    "random_graph": (lambda: C.random_graph(), {}),
}


def _engine(m, passes=3, **kw):
    e = E.Engine(0)
    e.upload(m, **kw)
    e.set_reparametrization(ANISO)
    if passes:
        e.compute_pass(passes)
    return e


def _check_all(e, m, what):
    """every direction and refinement count against the reference on the engine's own duals; returns the number of decodes"""
    duals = e.download_duals()
    assert not np.any(np.isnan(duals)), what
    n = 0
    for d in (0, 1):
        order = e.plan.order(d)
        for refine in (0, 1, 3):
            e.decode_primal(d, refine)
            got = e.download_primal()
            want = C.decode_reference(m, duals, order, refine)
            bad = np.argwhere(got != want)
            assert np.array_equal(got, want), (what, d, refine, bad[:8].tolist(), got[bad[:8, 0]].tolist(), want[bad[:8, 0]].tolist())
            n += 1
    return n


@pytest.mark.parametrize("name", sorted(CASES))
def test_decode_matches_the_reference(name):
    make, kw = CASES[name]
    m = make()
    e = _engine(m, **kw)
    if "rows_layout" in kw:
        assert e.rows_layout
    if "table_precision" in kw:
        assert e.table_precision() == kw["table_precision"]
    assert _check_all(e, m, name) == 6
    e.close()


def test_all_inf_unary_takes_label_zero_and_ties_take_the_first():
    m = C.mixed_case()
    e = _engine(m)
    e.decode_primal(0, 0)
    pr = e.download_primal()
    assert pr[9, 0] == 0 and np.all(np.isinf(m.dual_data[m.dual_offsets()[9]:m.dual_offsets()[10]]))
    e.close()
    # constant costs everywhere: every c is constant, every label 0
    un = [np.full(5, 2.0) for _ in range(3)]
    m = C.build_model(un, [(0, 1, ("dense", np.full((5, 5), 1.0))), (1, 2, ("potts", 0.0))])
    e = _engine(m)
    for d in (0, 1):
        e.decode_primal(d, 1)
        assert not e.download_primal().any()
    e.close()


def test_decode_reads_only():
    """duals and the tracked bound are bit-identical before and after; the decode makes no bound stale"""
    for make, kw in ((lambda: C.grid(9, 7, 8, "colour_major"), {}), (lambda: C.labels_case(13), {"rows_layout": True}), (lambda: C.mixed_case(), {})):
        m = make()
        e = _engine(m, **kw)
        lb0 = e.lower_bound()
        rec0 = e.lower_bound_recomputed()
        d0 = e.download_duals()
        lb0b = e.lower_bound()
        rec0b = e.lower_bound_recomputed()
        for d in (0, 1):
            e.decode_primal(d, 2)
        lb1 = e.lower_bound()
        rec1 = e.lower_bound_recomputed()
        d1 = e.download_duals()
        assert d0.tobytes() == d1.tobytes()
        assert np.float64(lb0).tobytes() == np.float64(lb1).tobytes() == np.float64(lb0b).tobytes()
        print("bounds recomputed: after the passes", rec0, "again", rec0b, "after the decodes", rec1)
        assert rec1 <= rec0b
        # and a pass afterwards continues from the same duals as on an engine that never decoded
        f = _engine(m, **kw)
        e.compute_pass(1); f.compute_pass(1)
        assert np.array_equal(e.download_duals(), f.download_duals())
        e.close(); f.close()


@pytest.mark.parametrize("name", ["grid_colour_major", "mixed", "diff_banded", "dense_f32", "random_graph"])
def test_decoded_labels_are_consistent_and_cost_the_original_energy(name):
    make, kw = CASES[name]
    m = make()
    if name == "mixed":        # (without the all-+inf unary: its energy is +inf)
        m = dataclasses.replace(m, dual_data=np.where(np.isinf(m.dual_data), 1.0, m.dual_data), _keep=[])
    e = _engine(m, **kw)
    for d, refine in ((0, 0), (1, 2)):
        e.decode_primal(d, refine)
        assert e.check_primal_consistency()
        cost, want = e.evaluate_primal(), C.energy(m, e.download_primal())
        print(name, d, refine, "evaluate_primal", cost, "numpy energy", want, "lower bound", e.lower_bound())
        assert abs(cost - want) <= 1e-9 * max(1.0, abs(want))
        assert cost >= e.lower_bound() - 1e-9 * max(1.0, abs(cost))
    e.close()


def test_decode_after_new_costs_plans_nothing():
    A = RC.grid(9, 7, 8)
    B = RC.recost(A, 77)
    e = _engine(A)
    _check_all(e, A, "A")
    built = e.schedules_built()
    e.upload_costs(const=B.const_data, duals=B.dual_data)
    e.compute_pass(3)
    _check_all(e, B, "B")
    assert e.schedules_built() == built
    # pool values and listed constants keep the tables, too
    m = C.labels_case(13, "shared")
    e2 = _engine(m)
    _check_all(e2, m, "shared")
    built = e2.schedules_built()
    m2 = m.with_pool(m.sh_data * 0.5 + 0.25)
    e2.upload_shared_pool(m2.sh_data)
    _check_all(e2, m2, "shared, new pool")
    assert e2.schedules_built() == built
    # a new model drops them
    e2.upload(m)
    e2.set_reparametrization(ANISO)
    assert e2.schedules_built() <= built - 2
    e.close(); e2.close()


def test_decode_settles_passes_that_ran_ahead(monkeypatch):
    """with speculation on the device is passes ahead of the caller: the decode first settles (here a rollback, the caller stopped
    inside a batch) and reads the duals of the pass the caller is at"""
    monkeypatch.setenv("LPMP_ROT_BANDS", "6")          # the joined chain on a small model (as tests/test_speculation_gpu.py does)
    m = S.grid_model(40, 36, 32, order="colour_major", seed=6)
    e, f = E.Engine(0), E.Engine(0)
    for x in (e, f):
        x.upload(m); x.set_reparametrization(ANISO)
        x.lower_bound()
    e.set_speculation(8)
    for k in range(4):                                  # batches of 2 and 4: the caller is at pass 4 of 6
        e.compute_pass(1); f.compute_pass(1)
    st = e.speculation_stats()
    assert st["batches"] == 2 and st["passes_launched"] == 6 and st["rollbacks"] == 0, st
    e.decode_primal(0, 1); f.decode_primal(0, 1)
    assert e.speculation_stats()["rollbacks"] == 1
    got = e.download_primal()
    duals = e.download_duals()
    assert np.array_equal(duals, f.download_duals())
    assert np.array_equal(got, f.download_primal())
    assert np.array_equal(got, C.decode_reference(m, duals, e.plan.order(0), 1))
    e.close(); f.close()


def test_error_returns_and_the_lp_mirror():
    e = E.Engine(0)
    with pytest.raises(E.EngineError) as ei:
        e.decode_primal(0, 0)
    assert ei.value.code == ERR_STATE
    m = C.labels_case(13)
    e.upload(m)
    for args in ((2, 0), (-1, 0), (0, -1)):
        with pytest.raises(E.EngineError) as ei:
            e.decode_primal(*args)
        assert ei.value.code == ERR_INVALID
    e.decode_primal(0, 0)                       # no weights needed: the decode reads duals only
    assert e.check_primal_consistency()
    mc = S.multicut_triangle_model(6, 4, seed=1)
    e.upload(mc)
    with pytest.raises(E.EngineError) as ei:
        e.decode_primal(0, 0)
    assert ei.value.code == ERR_UNSUPPORTED and "factor" in str(ei.value)
    e.close()
    # LP mirror: the README quick-start model (optimum 1.0 at labels (0, 0) or (1, 1): the first minimiser gives (0, 0))
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.PairwiseSimplexFactor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    lp = LPM.LP(LPM.FMC("SRMP", [U, P], [ML, MR]))
    u1, u2 = lp.add_factor(U, [0.0, 1.0]), lp.add_factor(U, [1.0, 0.0])
    p = lp.add_factor(P, 2, 2, [[0.0, 1.0], [1.0, 0.0]])
    lp.add_message(ML, u1, p); lp.add_message(MR, u2, p)
    lp.AddFactorRelation(u1, p); lp.AddFactorRelation(p, u2)
    lp.set_reparametrization("anisotropic")
    lp.ComputePass(0)
    cost = lp.decode_primal(0, 1)
    pr = lp.primal()
    assert cost == 1.0 and lp.CheckPrimalConsistency() and pr[u1, 0] == pr[u2, 0] and list(pr[p]) == [pr[u1, 0], pr[u2, 0]]
    # a later rounding pass behaves as after upload_primal: same labels as on an engine that uploaded the decoded labels
    m = S.grid_model(9, 7, 8, order="colour_major", seed=5, compute_primal=True)
    a, b = _engine(m), _engine(m)
    a.decode_primal(0, 0)
    b.upload_primal(a.download_primal())
    a.compute_pass_and_primal(1); b.compute_pass_and_primal(1)
    assert np.array_equal(a.download_primal(), b.download_primal()) and np.array_equal(a.download_duals(), b.download_duals())
    a.close(); b.close()
