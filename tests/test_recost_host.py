"""Host side of "new costs on the plan that is already there" (no GPU): the ABI, the LP mirror's bookkeeping with the engine stubbed
out, the numpy statements the GPU tests compare against, and the premise itself — the planner does not read a cost."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import recost_cases as C                          # noqa: E402
import schedule_hazards as H                      # noqa: E402
from lp_mp_amd import build as B                  # noqa: E402
from lp_mp_amd import engine as E                 # noqa: E402
from lp_mp_amd import lp as LPM                   # noqa: E402
from lp_mp_amd import model as M                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lpmp_upload_costs", "lpmp_set_vectors", "lpmp_zero_pairwise_duals", "lpmp_schedules_built")


def test_abi_symbols():
    """declared in the public header, exported by the built library, bound with the prototypes of the header"""
    h = open(os.path.join(ROOT, "include", "lpmp_engine.h")).read()
    raw = ctypes.CDLL(B.build())
    L = E.lib()
    for fn in NEW:
        assert re.search(r"\b%s\(" % fn, h) and fn in E.EXPORTS
        assert getattr(raw, fn) is not None
    assert len(L.lpmp_upload_costs.argtypes) == 5 and len(L.lpmp_set_vectors.argtypes) == 7
    assert L.lpmp_schedules_built.restype is ctypes.c_int64
    # without an engine: the count is 0 and the calls fail by status, not by a crash
    assert L.lpmp_schedules_built(None) == 0
    assert L.lpmp_upload_costs(None, None, 0, None, 0) == -4 and b"no model" in L.lpmp_last_error()
    assert L.lpmp_zero_pairwise_duals(None) == -4
    for m in ("upload_costs", "set_vectors", "zero_pairwise_duals", "schedules_built"):
        assert callable(getattr(E.Engine, m))


# ---- the LP mirror with the engine stubbed out ------------------------------------------------------------------------------
class StubEngine:
    def __init__(self):
        self.calls = []

    def upload(self, model, **kw):
        self.model = model; self.calls.append(("upload",))

    def upload_costs(self, const=None, duals=None):
        self.calls.append(("upload_costs", None if const is None else np.array(const), None if duals is None else np.array(duals)))

    def set_vectors(self, factors, src, accumulate=False):
        self.calls.append(("set_vectors", list(factors), np.array(src), accumulate))

    def set_inner_iterations(self, n): pass
    def set_reparametrization_type(self, t): pass
    def set_speculation(self, n): pass
    def download_duals(self): return np.array(self.model.dual_data)


def _lp():
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.PairwiseSimplexFactor, 1)
    Q = LPM.FactorContainer(LPM.pairwise_potts_factor, 2)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    NL = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 2, M.SCHED_LEFT, M.variableMessageNumber, 1, 2)
    NR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 2, M.SCHED_LEFT, M.variableMessageNumber, 1, 3)
    lp = LPM.LP(LPM.FMC("SRMP+Potts", [U, P, Q], [ML, MR, NL, NR]))
    u = [lp.add_factor(U, c) for c in ([0.0, 1.0], [1.0, 0.0, 0.5], [0.25, 0.75, 0.5])]
    p = lp.add_factor(P, 2, 3, np.arange(6.0).reshape(2, 3))
    q = lp.add_factor(Q, 3, 0.5)
    lp.add_message(ML, u[0], p); lp.add_message(MR, u[1], p); lp.add_message(NL, u[1], q); lp.add_message(NR, u[2], q)
    lp.AddFactorRelation(u[0], p); lp.AddFactorRelation(p, u[1]); lp.AddFactorRelation(u[1], q); lp.AddFactorRelation(q, u[2])
    lp._engine = StubEngine()
    return lp, u, p, q


def test_set_factor_cost_and_the_dirty_flag():
    lp, u, p, q = _lp()
    eng = lp._engine
    lp.upload_costs()                                   # dirty: the ordinary upload
    assert [c[0] for c in eng.calls] == ["upload"] and not lp._dirty
    first = lp._model
    lp.set_factor_cost(u[1], [2.0, 0.0, 0.5])
    lp.set_factor_cost(p, 2, 3, np.ones((2, 3)))
    lp.set_factor_cost(q, 3, 0.125)
    assert not lp._dirty
    lp.upload_costs()                                   # clean: new numbers on the planned model
    name, const, duals = eng.calls[-1]
    assert name == "upload_costs" and len(eng.calls) == 2
    want = lp.flat_model()
    assert np.array_equal(const, want.const_data) and np.array_equal(duals, want.dual_data)
    assert np.array_equal(const, np.concatenate([np.ones(6), [0.125]]))
    off = want.dual_offsets()
    assert np.array_equal(duals[off[u[1]]:off[u[1] + 1]], [2.0, 0.0, 0.5]) and np.all(duals[~C.vector_mask(want)] == 0.0)
    for a in ("f_kind", "f_dim0", "f_dim1", "m_left", "m_right", "rel_fwd"):
        assert np.array_equal(getattr(first, a), getattr(want, a))
    # warm: constants only, and new - old for the unaries that changed
    lp.set_factor_cost(u[0], [0.5, 1.0])
    lp.set_factor_cost(p, 2, 3, np.zeros((2, 3)))
    lp.upload_costs(warm=True)
    (n1, c1, d1), (n2, fs, src, acc) = eng.calls[-2:]
    assert n1 == "upload_costs" and d1 is None and np.array_equal(c1, np.concatenate([np.zeros(6), [0.125]]))
    assert n2 == "set_vectors" and acc and fs == [u[0]] and np.array_equal(src, [[0.5, 0.0]])
    # a structural call: the ordinary upload again
    lp.add_to_constant(1.0)
    assert lp._dirty
    lp.upload_costs()
    assert eng.calls[-1] == ("upload",)
    # shape or kind may not change
    for bad in ((u[0], [0.0, 1.0, 2.0]), (p, 3, 2, np.zeros((3, 2))), (q, 4, 0.5)):
        with pytest.raises(RuntimeError):
            lp.set_factor_cost(*bad)
    with pytest.raises(RuntimeError):
        lp.set_factor_cost(p, LPM.PairwiseSimplexFactor(2, 2))
    assert not lp._dirty


def test_warm_differences_are_taken_to_costs_also_after_a_structural_change():
    """solve, add a factor (the mirror pulls the device's reparametrised duals and lays them over the next upload), solve, change ONE
    unary, warm: exactly that row goes out, as new - old COST — not cost minus whatever dual was pulled"""
    lp, u, p, q = _lp()
    eng = lp._engine
    lp.upload_costs()
    eng.download_duals = lambda: np.array(eng.model.dual_data) + 7.0        # what a solve leaves: not the costs
    U = lp.FMC.FactorList[0]
    extra = lp.add_factor(U, [0.5, 0.25])                                    # structural: pulls the duals, marks the LP dirty
    assert lp._dirty and lp._duals_host is not None
    lp.upload_costs()                                                        # the ordinary upload, pulled duals laid over the costs
    assert eng.calls[-1] == ("upload",) and not lp._dirty
    off = lp._model.dual_offsets()
    assert np.array_equal(lp._model.dual_data[off[u[0]]:off[u[0] + 1]], [7.0, 8.0])          # the uploaded duals are the pulled ones
    assert np.array_equal(lp._cost_dual[off[u[0]]:off[u[0] + 1]], [0.0, 1.0])                # ... the costs are kept beside them
    assert np.array_equal(lp._cost_dual[off[extra]:off[extra + 1]], [0.5, 0.25])
    lp.set_factor_cost(u[2], [0.25, 1.75, 0.0])
    n = len(eng.calls)
    lp.upload_costs(warm=True)
    sent = eng.calls[n:]
    assert [c[0] for c in sent] == ["upload_costs", "set_vectors"] and sent[0][2] is None
    _, fs, src, acc = sent[1]
    assert acc and fs == [u[2]] and np.array_equal(src, [[0.0, 1.0, -0.5]])
    lp.upload_costs(warm=True)                                               # nothing changed since: no row goes out
    assert [c[0] for c in eng.calls[n + 2:]] == ["upload_costs"]


# ---- the numpy statements the GPU tests use ---------------------------------------------------------------------------------
def test_numpy_statements_follow_the_flat_model_offsets():
    m = C.vector_lengths_model()
    off = m.dual_offsets()
    vm = C.vector_mask(m)
    vec = np.flatnonzero(m.f_kind == M.F_VECTOR)
    assert vm.shape[0] == m.dual_data.shape[0] == off[-1]
    for f in range(m.n_factors):
        assert np.all(vm[off[f]:off[f + 1]] == (m.f_kind[f] == M.F_VECTOR))
    rows = np.arange(len(vec) * 310.0).reshape(len(vec), 310) + 1000.0
    d = C.scatter_rows(m, m.dual_data, vec[::-1], rows)
    for i, f in enumerate(vec[::-1]):
        assert np.array_equal(d[off[f]:off[f + 1]], rows[i, :m.f_dim0[f]])
    assert np.array_equal(d[~vm], m.dual_data[~vm])
    d2 = C.scatter_rows(m, d, vec[:2], rows, accumulate=True)
    n0 = m.f_dim0[vec[0]]
    assert np.array_equal(d2[off[vec[0]]:off[vec[0] + 1]], rows[len(vec) - 1, :n0] + rows[0, :n0])
    assert np.array_equal(d2[off[vec[2]]:], d[off[vec[2]]:])
    z = C.zero_pairwise(m, np.full(off[-1], -3.0))
    assert np.all(z[vm] == -3.0) and np.all(z[~vm] == 0.0) and not np.any(np.signbit(z[~vm]))
    # recost: the same structure, other numbers, the pool untouched
    for A in (C.grid(7, 6, 13), C.shared_grid(), C.diff_grid(40, True), C.grid(7, 6, 8, "colour_major", "potts"), C.c5_small()):
        Bm = C.recost(A, 505)
        assert Bm.const_data.shape == A.const_data.shape and Bm.dual_data.shape == A.dual_data.shape
        assert np.all(Bm.dual_data[~C.vector_mask(A)] == 0.0)
        assert not np.array_equal(Bm.dual_data, A.dual_data)
        for a in ("f_kind", "f_dim0", "f_dim1", "f_type", "m_type", "m_left", "m_right", "rel_fwd", "rel_bwd", "sh_data", "f_table"):
            x, y = getattr(A, a), getattr(Bm, a)
            assert (x is None and y is None) or np.array_equal(x, y)
    Bf = C.recost(C.grid(7, 6, 13), 5, float_valued=True)
    assert np.array_equal(Bf.const_data.astype(np.float32).astype(np.float64), Bf.const_data)


# ---- the premise: schedules do not read costs -------------------------------------------------------------------------------
def _summary(m, table_precision=None):
    p = E.Plan(m, table_precision=table_precision)
    out = {}
    for name, mode in (("anisotropic", M.REPAM_ANISOTROPIC), ("uniform", M.REPAM_UNIFORM)):
        out[name] = {"schedule_classes": [p.schedule_classes(d, mode) for d in (0, 1)],
                     "schedule_info": [p.schedule_info(d, mode) for d in (0, 1)],
                     "chain_info": [p.chain_info(d, mode) for d in (0, 1, -1)],
                     "pass_rotates": p.pass_rotates(mode)}
    if m.has_diff:
        out["diff_bands"] = p.diff_bands()
        out["diff_band_info"] = [p.diff_band_info(d, M.REPAM_ANISOTROPIC) for d in (0, 1)]
    return out


PLANNED = {
    "dense colour-major": (lambda: C.grid(7, 6, 32), None),
    "dense row-major (mailbox chain)": (C.mailbox_grid, None),
    "dense, float tables": (lambda: C.grid(7, 6, 13), "f32"),
    "shared": (C.shared_grid, None),
    "diff banded": (lambda: C.diff_grid(40, True), None),
    "diff unbanded": (lambda: C.diff_grid(13, False), None),
}


@pytest.fixture(scope="module")
def probe_lib(tmp_path_factory):
    return H.build_probe(tmp_path_factory.mktemp("schedule_probe"))


@pytest.mark.parametrize("name", list(PLANNED))
def test_plans_do_not_depend_on_costs(name, probe_lib):
    """planning model A and model B gives the same summaries and, through the probe library, the same schedule word for word
    (records, ops with their weights, launches, chains, tickets, dependencies, mailbox rows): what lpmp_upload_costs keeps is what a
    fresh upload of B would plan again"""
    make, prec = PLANNED[name]
    A = make()
    Bm = C.recost(A, 77)
    assert not np.array_equal(A.dual_data, Bm.dual_data)
    assert _summary(A, prec) == _summary(Bm, prec)
    pa, pb = E.Plan(A, table_precision=prec), E.Plan(Bm, table_precision=prec)
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        segs = []
        for p in (pa, pb):
            rows = []
            for d in (0, 1):
                oo, om = p.omega(d, mode); mo, mk = p.mask(d, mode)
                rows.append((p.update_order(d), oo, om, mo, mk))
            segs.append(rows)
        for x, y in zip(segs[0], segs[1]):
            assert all(np.array_equal(a, b) for a, b in zip(x, y))
        for fuse, which in ((False, [0]), (False, [1]), (True, [0, 1])):
            SA = H.Probe(probe_lib, A).plan([segs[0][k] for k in which], fuse=fuse)
            SB = H.Probe(probe_lib, Bm).plan([segs[1][k] for k in which], fuse=fuse)
            assert len(SA["rec_factor"]) > 0
            chains_a, chains_b = SA.pop("chains"), SB.pop("chains")
            assert sorted(SA) == sorted(SB)
            for k in SA:
                assert SA[k].tobytes() == SB[k].tobytes(), (name, mode, fuse, k)
            assert len(chains_a) == len(chains_b)
            for ca, cb in zip(chains_a, chains_b):
                for k in ca:
                    assert ca[k].tobytes() == cb[k].tobytes(), (name, mode, fuse, k)
