"""Host side of "new pairwise parameters on the plan that is already there" (no GPU): lpmp_plan_set_shared_pool re-detects the bands
of DIFF vectors and the kernel choice of every cached launch of class diff and moves nothing else; FlatModel.with_pool and the LP
mirror's pool bookkeeping."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import repool_cases as R                          # noqa: E402
from lp_mp_amd import build as B                  # noqa: E402
from lp_mp_amd import engine as E                 # noqa: E402
from lp_mp_amd import lp as LPM                   # noqa: E402
from lp_mp_amd import model as M                  # noqa: E402
from lp_mp_amd import synthetic as S              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANISO, UNIFORM = M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM
NEW = ("lpmp_plan_set_shared_pool", "lpmp_upload_shared_pool", "lpmp_set_constants")


def test_abi_symbols():
    h = open(os.path.join(ROOT, "include", "lpmp_engine.h")).read()
    raw = ctypes.CDLL(B.build())
    L = E.lib()
    for fn in NEW:
        assert re.search(r"\b%s\(" % fn, h) and fn in E.EXPORTS
        assert getattr(raw, fn) is not None
    assert len(L.lpmp_plan_set_shared_pool.argtypes) == 2 and len(L.lpmp_upload_shared_pool.argtypes) == 3
    assert len(L.lpmp_set_constants.argtypes) == 6
    # without an engine: by status, not by a crash
    assert L.lpmp_upload_shared_pool(None, None, 0) == -4 and b"no model" in L.lpmp_last_error()
    assert L.lpmp_set_constants(None, 0, None, None, 0, 0) == -4
    assert L.lpmp_plan_set_shared_pool(None, None) == -1
    for m in ("upload_shared_pool", "set_constants"):
        assert callable(getattr(E.Engine, m))
    assert callable(E.Plan.set_shared_pool) and callable(M.FlatModel.with_pool)


def _state(p, modes=(ANISO, UNIFORM)):
    """everything of a plan a pool swap may NOT move, and what it may"""
    fixed = {m: ([p.schedule_info(d, m) for d in (0, 1)], [p.schedule_classes(d, m) for d in (0, 1)], p.pass_schedule_info(m),
                 [p.chain_info(d, m) for d in (0, 1, -1)]) for m in modes}
    band = {m: [p.diff_band_info(d, m) for d in (0, 1)] for m in modes}
    return fixed, band, p.diff_bands()


@pytest.mark.parametrize("order", ["colour_major", "row_major"])
def test_band_follows_the_pool_and_nothing_else_moves(order):
    L = 40
    A = R.diff_grid(L, order)
    D0, D1 = R.tl(L, R.BANDED), R.tl(L, R.UNBANDED)
    assert M.diff_band_is_banded(D0) and not M.diff_band_is_banded(D1)
    p = E.Plan(A)
    fixed0, band0, bands0 = _state(p)
    for m in band0:
        for bi in band0[m]:
            assert bi["band_launches"] == bi["diff_launches"] > 0 and bi["band_receives"] == bi["diff_receives"]
    assert bands0 == {0: M.diff_band(D0) + (True,)}
    Bm = A.with_pool(D1)
    p.set_shared_pool(Bm.sh_data)
    fixed1, band1, bands1 = _state(p)
    assert fixed1 == fixed0                                     # levels, launches, records, classes, bytes, chains: the same
    for m in band1:
        for b0, b1 in zip(band0[m], band1[m]):
            assert b1["band_launches"] == 0 and b1["band_receives"] == 0
            assert b1["diff_launches"] == b0["diff_launches"] and b1["diff_receives"] == b0["diff_receives"]
    assert bands1 == {0: M.diff_band(D1) + (False,)}
    q = E.Plan(Bm)                                              # the plan a fresh upload of the new pool would make
    assert _state(q) == (fixed1, band1, bands1)
    p.set_shared_pool(A.sh_data)                                # and back: the original state
    assert _state(p) == (fixed0, band0, bands0)


def test_launch_rule_is_all_receives_banded():
    """two vectors, alternating over the edges: every launch of a colour-major grid receives through both.  One vector unbanded is
    enough to take every launch off the banded kernel; the other one keeps its own band state"""
    L = 40
    A = R.diff_grid(L, "colour_major", n_tables=2)
    D0, D2, D1 = R.tl(L, R.BANDED), R.tl(L, R.BANDED_2), R.tl(L, R.UNBANDED)
    assert M.diff_band_is_banded(D2) and M.diff_band(D2) != M.diff_band(D0)
    p = E.Plan(A)
    n = p.diff_band_info(0, ANISO)["diff_launches"]
    assert p.diff_band_info(0, ANISO)["band_launches"] == n > 0
    p.set_shared_pool(np.stack([D0, D1]))
    assert p.diff_bands() == {0: M.diff_band(D0) + (True,), 1: M.diff_band(D1) + (False,)}
    for d in (0, 1):
        assert p.diff_band_info(d, ANISO) == E.Plan(A.with_pool(np.stack([D0, D1]))).diff_band_info(d, ANISO)
        assert p.diff_band_info(d, ANISO)["band_launches"] == 0
    p.set_shared_pool(np.stack([D2, D0]))                       # both banded again, other widths
    assert p.diff_bands() == {0: M.diff_band(D2) + (True,), 1: M.diff_band(D0) + (True,)}
    assert p.diff_band_info(0, ANISO)["band_launches"] == n
    # row-major, vectors by anti-diagonal (tests/mixed_precision_cases.py): launches that reference ONE vector each follow their own
    import mixed_precision_cases as MP
    m = MP.m1(("diff",), False)
    pm = E.Plan(m)
    b0 = pm.diff_band_info(0, ANISO)
    assert 0 < b0["band_launches"] < b0["diff_launches"]
    Lm = MP.LABELS["diff"]
    pm.set_shared_pool(np.stack([R.tl(Lm, R.UNBANDED), R.tl(Lm, R.BANDED)]))     # the roles swapped
    b1 = pm.diff_band_info(0, ANISO)
    assert b1["diff_launches"] == b0["diff_launches"] and 0 < b1["band_launches"] < b1["diff_launches"]
    assert b1 == E.Plan(m.with_pool(np.stack([R.tl(Lm, R.UNBANDED), R.tl(Lm, R.BANDED)]))).diff_band_info(0, ANISO)
    pm.set_shared_pool(np.stack([R.tl(Lm, R.BANDED), R.tl(Lm, R.BANDED_2)]))
    assert pm.diff_band_info(0, ANISO)["band_launches"] == b0["diff_launches"]


def test_shared_only_model_has_no_band_state():
    A = R.shared_grid_small(13)
    p = E.Plan(A)
    fixed0, band0, bands0 = _state(p, (ANISO,))
    assert bands0 == {} and band0[ANISO][0]["diff_launches"] == 0
    p.set_shared_pool(R.pool_of(A, 3, inf_at=5))                # +inf is allowed, as at the upload
    assert _state(p, (ANISO,)) == (fixed0, band0, {})


def test_refusals_leave_the_plan_as_it_was():
    A = R.diff_grid(40, "colour_major")
    p = E.Plan(A)
    before = _state(p)
    bad = np.array(R.tl(40, R.UNBANDED), copy=True)
    bad[17] = np.nan
    with pytest.raises(E.EngineError, match=r"table 0\b.*NaN") as ei:
        p.set_shared_pool(bad)
    assert ei.value.code == -1 and _state(p) == before
    with pytest.raises(E.EngineError) as ei:
        p.set_shared_pool(None)
    assert ei.value.code == -1 and _state(p) == before
    # a plan without a pool
    q = E.Plan(S.grid_model(4, 3, 4, order="colour_major"))
    with pytest.raises(E.EngineError) as ei:
        q.set_shared_pool(np.zeros(3))
    assert ei.value.code == -1


def test_no_diff_band_stays_what_it_was_when_the_plan_was_made(monkeypatch):
    A = R.diff_grid(40, "colour_major")
    monkeypatch.setenv("LPMP_NO_DIFF_BAND", "1")
    p = E.Plan(A)
    monkeypatch.delenv("LPMP_NO_DIFF_BAND")
    assert p.diff_band_info(0, ANISO)["band_launches"] == 0 and p.diff_bands()[0][2]
    p.set_shared_pool(R.tl(40, R.BANDED_2))
    assert p.diff_bands() == {0: M.diff_band(R.tl(40, R.BANDED_2)) + (True,)}
    bi = p.diff_band_info(0, ANISO)
    assert bi["band_launches"] == 0 and bi["diff_launches"] > 0


def test_with_pool():
    A = R.diff_grid(40, "colour_major", n_tables=2)
    new = np.stack([R.tl(40, R.UNBANDED), R.tl(40, R.BANDED_2)])
    Bm = A.with_pool(new)
    assert np.array_equal(Bm.sh_data, new.reshape(-1)) and Bm.sh_data is not A.sh_data
    assert np.array_equal(A.sh_data, np.stack([R.tl(40, R.BANDED)] * 2).reshape(-1))        # A is not modified
    for a in ("f_kind", "f_dim0", "f_dim1", "f_table", "sh_off", "sh_dim0", "sh_dim1", "const_data", "dual_data", "m_left", "m_right"):
        assert getattr(Bm, a) is getattr(A, a) or np.array_equal(getattr(Bm, a), getattr(A, a))
    assert np.array_equal(Bm.expand_diff().const_data[:40 * 40],
                          (np.float64(Bm.const_data[0]) * M.truncated_linear(40, 40, *R.UNBANDED)[np.subtract.outer(np.arange(40), np.arange(40)) + 39]).reshape(-1))
    with pytest.raises(ValueError):
        A.with_pool(new.reshape(-1)[:-1])
    bad = new.copy(); bad[1, 3] = np.nan
    with pytest.raises(ValueError):
        A.with_pool(bad)
    with pytest.raises(ValueError):
        S.grid_model(4, 3, 4).with_pool(np.zeros(3))


# ---- the LP mirror with the engine stubbed out ------------------------------------------------------------------------------
class StubEngine:
    def __init__(self):
        self.calls = []

    def upload(self, model, **kw):
        self.model = model; self.calls.append(("upload",))

    def upload_costs(self, const=None, duals=None):
        self.calls.append(("upload_costs", None if const is None else np.array(const), None if duals is None else np.array(duals)))

    def upload_shared_pool(self, sh_data):
        self.calls.append(("upload_shared_pool", np.array(sh_data)))

    def set_vectors(self, factors, src, accumulate=False):
        self.calls.append(("set_vectors", list(factors), np.array(src), accumulate))

    def set_constants(self, factors, src):
        self.calls.append(("set_constants", list(factors), np.array(src)))

    def set_inner_iterations(self, n): pass
    def set_reparametrization_type(self, t): pass
    def set_speculation(self, n): pass
    def download_duals(self): return np.array(self.model.dual_data)


def _lp():
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.PairwiseSimplexFactor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    lp = LPM.LP(LPM.FMC("mixed", [U, P], [ML, MR]))
    tv = lp.add_shared_table(np.arange(6.0).reshape(2, 3))
    td = lp.add_diff_table(np.arange(5.0))
    u = [lp.add_factor(U, c) for c in ([0.0, 1.0], [1.0, 0.0, 0.5], [0.25, 0.75, 0.5])]
    p = [lp.add_factor(P, 2, 3, np.ones((2, 3))), lp.add_factor(P, 3, 3, np.zeros((3, 3)))]
    lp.add_message(ML, u[0], p[0]); lp.add_message(MR, u[1], p[0]); lp.add_message(ML, u[1], p[1]); lp.add_message(MR, u[2], p[1])
    for a, b in ((u[0], p[0]), (p[0], u[1]), (u[1], p[1]), (p[1], u[2])):
        lp.AddFactorRelation(a, b)
    d = lp.add_factor(P, LPM.diff_pairwise_factor(td, 3, 3, 2.0))
    lp.add_message(ML, u[1], d); lp.add_message(MR, u[2], d)
    lp.AddFactorRelation(u[1], d); lp.AddFactorRelation(d, u[2])
    lp._engine = StubEngine()
    return lp, (tv, td), u, p, d


def test_lp_pool_bookkeeping():
    lp, (tv, td), u, p, d = _lp()
    eng = lp._engine
    lp.upload_costs()
    assert [c[0] for c in eng.calls] == ["upload"] and not lp._dirty
    op = lp.GetFactor(d)
    assert op.cost(2, 0) == 2.0 * 4.0
    lp.set_diff_table(td, [4.0, 3.0, 2.0, 1.0, 0.0])
    lp.set_shared_table(tv, np.full((2, 3), 7.0))
    assert not lp._dirty                                        # not structural
    assert lp.GetFactor(d).cost(2, 0) == 2.0 * 0.0              # the factor object sees the new vector
    for bad in (lambda: lp.set_diff_table(td, np.zeros(4)), lambda: lp.set_shared_table(tv, np.zeros((3, 2))),
                lambda: lp.set_diff_table(tv, np.zeros(6)), lambda: lp.set_shared_table(td, np.zeros(5)),
                lambda: lp.set_diff_table(9, np.zeros(5)), lambda: lp.set_diff_table(td, [0, 1, np.nan, 3, 4])):
        with pytest.raises(RuntimeError):
            bad()
    assert not lp._dirty
    # cold: the pool first, then the whole arrays
    lp.upload_costs()
    assert [c[0] for c in eng.calls] == ["upload", "upload_shared_pool", "upload_costs"]
    assert np.array_equal(eng.calls[1][1], np.concatenate([np.full(6, 7.0), [4.0, 3.0, 2.0, 1.0, 0.0]]))
    # warm: only the pairwise factors whose constants differ, through set_constants; nothing for an unchanged pool
    lp.set_factor_cost(p[1], 3, 3, np.arange(9.0).reshape(3, 3))
    lp.set_factor_cost(d, LPM.diff_pairwise_factor(td, 3, 3, 0.25))
    lp.set_factor_cost(u[0], [0.5, 1.0])
    n = len(eng.calls)
    lp.upload_costs(warm=True)
    sent = eng.calls[n:]
    assert [c[0] for c in sent] == ["set_constants", "set_vectors"]
    _, fs, rows = sent[0]
    assert fs == [p[1], d] and rows.shape == (2, 9)
    assert np.array_equal(rows[0], np.arange(9.0)) and rows[1, 0] == 0.25 and np.all(rows[1, 1:] == 0.0)
    assert sent[1][1] == [u[0]] and sent[1][3]
    n = len(eng.calls)
    lp.upload_costs(warm=True)                                   # nothing changed since: nothing goes out
    assert eng.calls[n:] == []
    lp.set_diff_table(td, np.ones(5))
    lp.upload_costs(warm=True)
    assert [c[0] for c in eng.calls[n:]] == ["upload_shared_pool"]
    # a structural call: the ordinary upload, which carries the pool
    lp.add_to_constant(1.0)
    lp.set_diff_table(td, np.zeros(5))
    lp.upload_costs()
    assert eng.calls[-1] == ("upload",) and not lp._pool_changed
