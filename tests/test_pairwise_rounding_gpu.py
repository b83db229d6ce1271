"""Pairwise factors that round themselves on the device — every pairwise kind, storage mode and kernel class of
tests/pairwise_rounding_cases.py — against the CPU oracle on the dense expansion: labels and duals bit for bit after every rounding
sweep, the cost within 1e-9, and the numpy energy of the device's labels on the kind model's original costs.
tests/test_pairwise_rounding_host.py pins the yardstick and the census of the same list on the host."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pairwise_rounding_cases as PR              # noqa: E402
from test_primal_gpu import MODES, _same          # noqa: E402
from lp_mp_amd import engine as E                 # noqa: E402
from lp_mp_amd import model as M                  # noqa: E402
from oracle.binding import Oracle                 # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """one engine per table precision: f64, and float storage of the dense tables"""
    es = {None: E.Engine(0), "f32": E.Engine(0)}
    yield es
    for e in es.values():
        e.close()


def _start(engines, c, mode, rtype=0):
    eng = engines[c.precision]
    o = Oracle(c.yardstick)
    o.set_reparametrization_type(rtype); o.set_reparametrization(mode)
    eng.upload(c.model, table_precision=c.precision or "f64")
    eng.set_reparametrization_type(rtype); eng.set_reparametrization(mode)
    return eng, o


def _loop(eng, o, name, iterations=2):
    """the solver's loop: a rounding sweep forward, one backward, a plain pass — everything against the oracle after each sweep"""
    best = np.inf
    for it in range(iterations):
        eng.forward_pass_and_primal(it); o.ComputeForwardPassAndPrimal(it)
        best = min(best, _same(eng, o, (name, "forward", it)))
        eng.backward_pass_and_primal(it); o.ComputeBackwardPassAndPrimal(it)
        best = min(best, _same(eng, o, (name, "backward", it)))
        eng.compute_pass(1); o.ComputePass(1)
    lb = eng.lower_bound()
    assert np.isfinite(best), name
    assert best >= lb - 1e-9 * max(1.0, abs(lb)), (name, best, lb)
    return best


def _close(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b))


@pytest.mark.parametrize("name", [c.name for c in PR.CASES])
def test_rounding_sweeps_equal_the_oracle_on_the_expansion(engines, name):
    c = PR.BY_NAME[name]
    m = c.model
    for mode in MODES:
        eng, o = _start(engines, c, mode)
        _same(eng, o, (name, mode, "unset"))
        _loop(eng, o, (name, mode))
    # once per case (on the state the last weight mode left): the check that does not pass through the oracle ...
    pr = eng.download_primal()
    cost = eng.evaluate_primal()
    assert _close(PR.energy(m, pr), cost), (name, PR.energy(m, pr), cost)
    # ... the prepared read-out of the labels ...
    ro = eng.readout(None)
    try:
        assert np.array_equal(ro.labels(), pr[m.f_kind == M.F_VECTOR, 0]), name
    finally:
        ro.close()
    # ... and the time stamps: the stamp of the last backward sweep keeps the labels, a later one rounds again
    eng.compute_pass(1); o.ComputePass(1)
    eng.backward_pass_and_primal(1); o.ComputeBackwardPassAndPrimal(1)
    assert np.array_equal(eng.download_primal(), pr), name
    _same(eng, o, (name, "same stamp"))
    eng.forward_pass_and_primal(2); o.ComputeForwardPassAndPrimal(2)
    _same(eng, o, (name, "later stamp"))
    eng.set_reparametrization_type(0)


KIND_CASES = PR.per_kind(8) + PR.per_kind(40)


@pytest.mark.parametrize("name", [c.name for c in KIND_CASES])
def test_rounding_sweeps_send_shared_under_the_residual_rule(engines, name):
    """primal passes always send `shared` (reference factors_messages.hxx:2357-2359); the plain pass in between follows the residual
    rule — on the generic kernels that run the rerouted launches, and on the class kernels of the unaries"""
    c = PR.BY_NAME[name]
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_DAMPED_UNIFORM):
        eng, o = _start(engines, c, mode, rtype=M.RTYPE_RESIDUAL)
        try:
            _loop(eng, o, (name, mode, "residual"))
        finally:
            eng.set_reparametrization_type(0)


# the adaptive rule: `full` with everything rounding, and `right` with only the pairwise type rounding (the unaries send nothing)
ADAPTIVE_CASES = KIND_CASES + PR.per_kind(8, sched="right", computes=(0, 1)) + PR.per_kind(40, sched="right", computes=(0, 1))


@pytest.mark.parametrize("name", [c.name for c in ADAPTIVE_CASES])
def test_rounding_sweeps_send_shared_under_the_adaptive_rule(engines, name):
    """RTYPE_ADAPTIVE rebuilds every schedule on the generic / lane-per-factor kernels (the rule lives there): rounding unaries
    then go through the generic kernel's store_label next to pairwise factors that round themselves.  The message types carry
    MF_IMPROVEMENT, so the adaptive weights of the plain pass in between are not all zero; the rounding sweeps send `shared`.
    The rule is defined where every message of an updated factor sends (Plan::adaptive_obstacle): where the oracle refuses
    the model, the engine must refuse it too — asserted, nothing is skipped."""
    c = dataclasses.replace(PR.BY_NAME[name], flags=M.MF_IMPROVEMENT)
    sends = 0
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_DAMPED_UNIFORM):
        eng = engines[c.precision]
        o = Oracle(c.yardstick)
        eng.upload(c.model, table_precision=c.precision or "f64")
        try:
            o.set_reparametrization_type(M.RTYPE_ADAPTIVE)
        except RuntimeError:
            with pytest.raises(E.EngineError) as ei:
                eng.set_reparametrization_type(M.RTYPE_ADAPTIVE)
            assert ei.value.code == -2                          # LPMP_ERR_UNSUPPORTED
            continue
        try:
            eng.set_reparametrization_type(M.RTYPE_ADAPTIVE)
            o.set_reparametrization(mode); eng.set_reparametrization(mode)
            for d in (M.FORWARD, M.BACKWARD):
                assert set(eng.plan.schedule_classes(d, mode)) <= {"generic", "small"}, (name, mode)
            _loop(eng, o, (name, mode, "adaptive"))
            sends += o.counters()[1]
        finally:
            eng.set_reparametrization_type(0)
    assert sends > 0, name                                      # (no model of the list is refused: the rule did run)


@pytest.mark.parametrize("name", [c.name for c in KIND_CASES])
def test_preset_labels_count_at_their_stamp_and_go_at_a_later_one(engines, name):
    """upload_primal with some unaries labelled (their factors' slots with them) and the others unset: a sweep of the stamp the
    engine is at keeps the given labels and the pairwise factors fill in round them; a sweep of a NEW stamp re-initialises what it
    touches — both as the oracle does (Oracle.set_primal).  A full labelling evaluates to its numpy energy."""
    c = PR.BY_NAME[name]
    m = c.model
    rng = np.random.default_rng(3)
    n = int(np.sum(m.f_kind == M.F_VECTOR))
    eng, o = _start(engines, c, M.REPAM_ANISOTROPIC)
    eng.forward_pass_and_primal(5); o.ComputeForwardPassAndPrimal(5)           # both are at stamp 11 now
    for on in ([k % 3 == 0 for k in range(n)], [k % 2 == 1 for k in range(n)]):
        pr = PR.consistent_preset(m, on, rng)
        eng.upload_primal(pr); o.set_primal(pr, 11)
        _same(eng, o, (name, "uploaded"))
        eng.forward_pass_and_primal(5); o.ComputeForwardPassAndPrimal(5)
        _same(eng, o, (name, "same stamp"))
        got = eng.download_primal()
        given = np.flatnonzero(m.f_kind == M.F_VECTOR)[np.asarray(on)]
        assert np.array_equal(got[given, 0], pr[given, 0]), name
        assert eng.check_primal_consistency()
        eng.compute_pass(1); o.ComputePass(1)
    pr = PR.consistent_preset(m, [k % 2 == 0 for k in range(n)], rng)
    eng.upload_primal(pr); o.set_primal(pr, 11)
    eng.forward_pass_and_primal(6); o.ComputeForwardPassAndPrimal(6)           # a new stamp
    _same(eng, o, (name, "new stamp"))
    full = PR.consistent_preset(m, [True] * n, rng)
    eng.upload_primal(full)
    assert eng.check_primal_consistency()
    assert _close(eng.evaluate_primal(), PR.energy(m, full)), (name, eng.evaluate_primal(), PR.energy(m, full))


@pytest.mark.parametrize("name", [c.name for c in KIND_CASES])
def test_kind_against_its_expansion_on_the_device(engines, name):
    """the engine on the kind model and a second engine on its dense expansion: equal labels and duals after the loop"""
    c = PR.BY_NAME[name]
    other = E.Engine(0)
    try:
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            eng, o = _start(engines, c, mode)
            other.upload(c.yardstick); other.set_reparametrization(mode)
            for it in range(2):
                for e in (eng, other):
                    e.forward_pass_and_primal(it); e.backward_pass_and_primal(it); e.compute_pass(1)
                assert np.array_equal(eng.download_primal(), other.download_primal()), (name, mode, it)
                assert np.array_equal(eng.download_duals(), other.download_duals()), (name, mode, it)
    finally:
        other.close()


def test_a_257_x_256_factor_is_refused_not_run(engines):
    """d0 + d1 = 513 is one more than the generic kernel holds (GEN_MAXD): set_reparametrization refuses the model"""
    eng = engines[None]
    eng.upload(PR.refused_model(), table_precision="f64")
    with pytest.raises(E.EngineError, match="exceeds the device limit") as ei:
        eng.set_reparametrization(M.REPAM_ANISOTROPIC)
    assert ei.value.code == -2                                 # LPMP_ERR_UNSUPPORTED
