"""Host side of the primal state calls (no GPU): the ABI of lpmp_readout_set_labels, lpmp_move_windows_carry, lpmp_lower_bound_dev and
lpmp_evaluate_primal_dev, and the numpy statement of the carried labels, ``lp_mp_amd.model.move_labels``: identity, unset entries,
the clamp at both ends, the energy kept bit for bit where nothing clamps (on the model and duals of ``model.move_windows``), and a
seeded wrong rule that every case tells apart."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import move_windows_cases as MW                   # noqa: E402
import primal_state_cases as C                    # noqa: E402
from lp_mp_amd import build as B                  # noqa: E402
from lp_mp_amd import engine as E                 # noqa: E402
from lp_mp_amd import lp as LPM                   # noqa: E402
from lp_mp_amd import model as M                  # noqa: E402
from oracle.binding import Oracle                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_symbols():
    """declared in the public header, exported by the built library, listed in E.EXPORTS, bound with the prototypes of the header;
    without an engine the calls fail by status, not by a crash"""
    h = open(os.path.join(ROOT, "include", "lpmp_engine.h")).read()
    raw = ctypes.CDLL(B.build())
    L = E.lib()
    for fn in C.NEW:
        assert re.search(r"\bint %s\(" % fn, h) and fn in E.EXPORTS
        assert getattr(raw, fn) is not None
    assert len(L.lpmp_readout_set_labels.argtypes) == 4 and len(L.lpmp_move_windows_carry.argtypes) == 8
    assert len(L.lpmp_lower_bound_dev.argtypes) == 2 and len(L.lpmp_evaluate_primal_dev.argtypes) == 2
    assert L.lpmp_readout_set_labels(None, None, None, 0) == C.INVALID
    assert L.lpmp_move_windows_carry(None, None, None, 0, None, None, 0, 0) == C.INVALID and b"lpmp_move_windows_carry" in L.lpmp_last_error()
    assert L.lpmp_lower_bound_dev(None, None) == C.STATE and L.lpmp_evaluate_primal_dev(None, None) == C.STATE
    assert callable(E.Readout.set_labels) and callable(M.move_labels)
    import inspect
    assert "carry_labels" in inspect.signature(E.WindowSet.move).parameters and "carry_labels" in inspect.signature(LPM.LP.move_windows).parameters
    assert "dst_dev" in inspect.signature(E.Engine.lower_bound).parameters and "dst_dev" in inspect.signature(E.Engine.evaluate_primal).parameters


# ---- lp_mp_amd.model.move_labels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", C.SHIFT_KEYS)
@pytest.mark.parametrize("which", C.LISTS)
def test_zero_is_the_identity_and_unset_stays_unset(key, which):
    m = C.shift_model(key)
    lst = C.listed(m, which)
    p = C.random_primal(m, 3, unset_every=4)
    u = C.unaries(m)
    was_unset = p[u, 0] == m.f_dim0[u]
    assert was_unset.any() and not was_unset.all()
    assert np.array_equal(M.move_labels(p, m, lst, C.deltas(m, lst, "zero")), p)
    for form in C.DELTA_FORMS:
        q = M.move_labels(p, m, lst, C.deltas(m, lst, form))
        assert np.array_equal(q[u, 0] == m.f_dim0[u], was_unset), form       # unset stays unset, set stays set
        assert np.all(q[u, 0] <= m.f_dim0[u]) and np.all(q[u, 0] >= 0)
        keep = np.setdiff1d(u, C.rows(m, lst))
        assert np.array_equal(q[keep], p[keep]), form                         # unlisted unaries keep their labels
        assert np.array_equal(q, C.propagate(m, q.copy())), form              # the pairwise slots follow the unaries that hold a label
    assert M.move_labels(p, m, lst, C.deltas(m, lst, "zero")) is not p and p.dtype == np.int32


@pytest.mark.parametrize("key", C.SHIFT_KEYS)
def test_the_clamp_at_both_ends(key):
    m = C.shift_model(key)
    u = C.unaries(m)
    d = m.f_dim0[u].astype(np.int64)
    p = C.random_primal(m, 5)
    delta = C.deltas(m, None, "clamp")
    q = M.move_labels(p, m, None, delta)
    assert np.array_equal(q[u, 0], np.where(delta > 0, 0, d - 1))             # everything clamps: delta >= d to label 0, <= -d to d - 1
    far = M.move_labels(p, m, None, C.deltas(m, None, "device_far"))
    want = np.clip(p[u, 0] - np.clip(C.deltas(m, None, "device_far"), -C.MOVE_DELTA_MAX, C.MOVE_DELTA_MAX), 0, d - 1)
    assert np.array_equal(far[u, 0], want)
    one = M.move_labels(p, m, None, C.deltas(m, None, "plus1"))
    assert np.array_equal(one[u, 0], np.maximum(p[u, 0] - 1, 0))
    one = M.move_labels(p, m, None, C.deltas(m, None, "minus1"))
    assert np.array_equal(one[u, 0], np.minimum(p[u, 0] + 1, d - 1))
    with pytest.raises(ValueError):
        M.move_labels(p, m, None, delta[:-1])
    with pytest.raises(ValueError):
        M.move_labels(p[:-1], m, None, delta)


def _after_passes(m, n=2):
    o = Oracle(MW.expand(m))
    o.set_reparametrization(M.REPAM_ANISOTROPIC)
    o.ComputePass(n)
    return o.duals()


@pytest.mark.parametrize("key", C.SHIFT_KEYS)
@pytest.mark.parametrize("which", C.LISTS)
@pytest.mark.parametrize("costs", (False, True))
def test_energy_is_kept_where_no_label_clamps(key, which, costs):
    """random deltas small enough that no label clamps: the energy of the carried labelling on the moved model and duals equals the
    energy before, term by term and as a sum, bit for bit — without costs and with costs that agree on the shared absolute labels.
    The wrong rule x + delta is told apart every time."""
    m = C.shift_model(key)
    lst = C.listed(m, which)
    d = _after_passes(m)
    for rep in range(4):
        p = C.random_primal(m, 10 + rep)
        delta = C.no_clamp_deltas(m, lst, p, 20 + rep)
        assert np.any(delta != 0)
        co, cn = C.agreeing_costs(m, lst, delta, 30 + rep) if costs else (None, None)
        m2, d2 = M.move_windows(m, d, lst, delta, co, cn)
        q = M.move_labels(p, m, lst, delta)
        f = C.rows(m, lst)
        assert np.array_equal(q[f, 0], p[f, 0] - delta)                       # nothing clamped
        before, after = C.energy_terms(m, d, p), C.energy_terms(m2, d2, q)
        assert before.tobytes() == after.tobytes(), int(np.sum(before != after))
        assert np.float64(C.energy(m, d, p)).tobytes() == np.float64(C.energy(m2, d2, q)).tobytes()
        w = C.wrong_move_labels(p, m, lst, delta)
        assert not np.array_equal(w, q)
        assert C.energy_terms(m2, d2, w).tobytes() != before.tobytes()


@pytest.mark.parametrize("key", C.SHIFT_KEYS)
@pytest.mark.parametrize("which", C.LISTS)
@pytest.mark.parametrize("form", [f for f in C.DELTA_FORMS if f != "zero"])
def test_the_wrong_rule_is_told_apart(key, which, form):
    m = C.shift_model(key)
    lst = C.listed(m, which)
    p = C.random_primal(m, 7, unset_every=5)
    delta = C.deltas(m, lst, form)
    assert not np.array_equal(C.wrong_move_labels(p, m, lst, delta), M.move_labels(p, m, lst, delta))


def test_a_model_the_rounding_code_refuses_moves_unaries_only():
    m, mg = C.lists_model()
    u = C.unaries(mg)[:6]
    p = C.unset_primal(m)
    p[u, 0] = [0, 1, 2, 3, 1, 2]
    q = M.move_labels(p, m, u, np.array([1, 1, -1, 0, -5, 5]))
    want = p.copy()
    want[u, 0] = [0, 0, 3, 3, 3, 0]
    assert np.array_equal(q, want)                                            # no pairwise slot is written


# ---- the LP mirror ---------------------------------------------------------------------------------------------------------------
class _StubSet:
    def __init__(self, eng, factors):
        self.eng, self.n = eng, len(factors)
        self.max_labels = max(int(eng.model.f_dim0[f]) for f in factors)

    def move(self, delta, cost_old=None, cost_new=None, carry_labels=False):
        self.eng.calls.append(("move", list(np.asarray(delta)), cost_old is not None, carry_labels))


class _StubEngine:
    def __init__(self):
        self.calls = []

    def upload(self, model, **kw):
        self.model = model

    def window_set(self, factors):
        return _StubSet(self, factors)

    def set_inner_iterations(self, n): pass
    def set_reparametrization_type(self, t): pass
    def set_speculation(self, n): pass

    def lower_bound(self, dst_dev=None):
        self.calls.append(("lower_bound", dst_dev))

    def evaluate_primal(self, dst_dev=None):
        self.calls.append(("evaluate_primal", dst_dev))


def test_lp_mirror_hands_the_new_arguments_on():
    """LP.move_windows(carry_labels=True) moves through the carrying call and keeps the same books; the scalars pass dst_dev on"""
    lp, u, p = MW.stub_window_lp()
    eng = lp._engine = _StubEngine()
    shifts = [lp.GetFactor(f).shift for f in p]
    lp.move_windows([u[1], u[2]], [1, -1], carry_labels=True)
    lp.move_windows([u[1], u[2]], [0, 1], new_costs=[np.zeros(6), np.ones(6)], carry_labels=True)
    lp.move_windows([u[1], u[2]], [0, 0])
    assert eng.calls == [("move", [1, -1], False, True), ("move", [0, 1], True, True), ("move", [0, 0], False, False)]
    assert [lp.GetFactor(f).shift for f in p] == [shifts[0] - 1, shifts[1] + 2 - 1, shifts[2] - 1 + 1]
    assert lp.LowerBound(dst_dev=4096) is None and lp.EvaluatePrimal(dst_dev=8192) is None
    assert eng.calls[-2:] == [("lower_bound", 4096), ("evaluate_primal", 8192)]
