"""Host side of lpmp_move_windows (no GPU): the ABI, the support check on a plan with every refusal naming its factor, the numpy
statement of the rule (``lp_mp_amd.model.move_windows``: identity, energy invariance on the dense expansion, saturation, the cost
rule), the oracle on a moved model, and the LP mirror's bookkeeping with the engine stubbed out."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import move_windows_cases as C                    # noqa: E402
from lp_mp_amd import build as B                  # noqa: E402
from lp_mp_amd import engine as E                 # noqa: E402
from lp_mp_amd import model as M                  # noqa: E402
from oracle.binding import Oracle                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lpmp_window_set_create", "lpmp_window_set_destroy", "lpmp_window_set_n", "lpmp_window_set_max_labels",
       "lpmp_window_set_n_pairwise", "lpmp_move_windows", "lpmp_plan_window_info")
INVALID, UNSUPPORTED, STATE = -1, -2, -4          # include/lpmp_engine.h


def test_abi_symbols():
    """declared in the public header, exported by the built library, bound with the prototypes of the header"""
    h = open(os.path.join(ROOT, "include", "lpmp_engine.h")).read()
    raw = ctypes.CDLL(B.build())
    L = E.lib()
    for fn in NEW:
        assert re.search(r"\b%s\(" % fn, h) and fn in E.EXPORTS
        assert getattr(raw, fn) is not None
    assert "typedef struct lpmp_window_set lpmp_window_set;" in h
    assert len(L.lpmp_move_windows.argtypes) == 8 and len(L.lpmp_plan_window_info.argtypes) == 7
    assert L.lpmp_window_set_n.restype is ctypes.c_int64 and L.lpmp_window_set_max_labels.restype is ctypes.c_int32
    # without an engine or a set: sizes are 0 and the calls fail by status, not by a crash
    assert L.lpmp_window_set_n(None) == 0 and L.lpmp_window_set_n_pairwise(None) == 0 and L.lpmp_window_set_max_labels(None) == 0
    out = ctypes.c_void_p()
    assert L.lpmp_window_set_create(None, 0, None, ctypes.addressof(out)) == STATE and b"no model" in L.lpmp_last_error()
    assert L.lpmp_move_windows(None, None, None, 0, None, None, 0, 0) == INVALID
    L.lpmp_window_set_destroy(None)
    for name in ("window_set",):
        assert callable(getattr(E.Engine, name))
    assert callable(E.Plan.window_info) and callable(E.WindowSet.move) and callable(M.move_windows)


# ---- the support check --------------------------------------------------------------------------------------------------------
def _refused(m, factors, code, names):
    with pytest.raises(E.EngineError) as ei:
        E.Plan(m).window_info(factors)
    assert ei.value.code == code, str(ei.value)
    assert names in str(ei.value), str(ei.value)
    # the numpy statement refuses the same list, for the same factor
    with pytest.raises(ValueError) as vi:
        M.window_links(m, factors)
    if code == UNSUPPORTED:
        assert isinstance(vi.value, M.WindowsUnsupported) and ("factor %d " % vi.value.factor) in str(ei.value)
    else:
        assert not isinstance(vi.value, M.WindowsUnsupported)


def test_window_info_counts():
    for L, order in ((5, "row_major"), (33, "colour_major")):
        m = C.grid(L, order)
        n_edges = C.D.n_edges(C.H, C.W)
        assert E.Plan(m).window_info() == dict(n_links=2 * n_edges, n_pairwise=n_edges)
        assert E.Plan(m).window_info(C.unaries(m)) == dict(n_links=2 * n_edges, n_pairwise=n_edges)
        assert E.Plan(m).window_info([]) == dict(n_links=0, n_pairwise=0)
    m, u, p, edges = C.edge_grid()
    # the corner has two edges, the centre four; listed together they share none
    assert E.Plan(m).window_info([u[0]]) == dict(n_links=2, n_pairwise=2)
    assert E.Plan(m).window_info([u[4], u[0]]) == dict(n_links=6, n_pairwise=6)
    assert E.Plan(m).window_info([u[0], u[1]]) == dict(n_links=5, n_pairwise=4)
    f, links, pairs = M.window_links(m, [u[0], u[1]])
    assert [len(l) for l in links] == [2, 3] and len(pairs) == 4
    e01 = p[edges.index((0, 1))]
    assert (e01, 0, 1) in pairs and sum(1 for q in pairs if q[1] >= 0 and q[2] >= 0) == 1


@pytest.mark.parametrize("other", ["dense", "potts", "diff"])
def test_refuses_a_peer_of_another_kind(other):
    m, u, p, edges = C.edge_grid(other)
    i, j = edges[4]
    assert m.f_kind[p[4]] != M.F_PAIRWISE_DIFF_SHIFT
    _refused(m, None, UNSUPPORTED, "factor %d " % u[i])                   # every vector: the lower end of the edge is named
    _refused(m, [u[j], u[i]], UNSUPPORTED, "factor %d " % u[i])
    _refused(m, [u[j]], UNSUPPORTED, "factor %d " % u[j])
    ok = [int(v) for v in u if v not in (u[i], u[j])]                     # the rest of the model may be anything
    assert E.Plan(m).window_info(ok)["n_links"] == sum(1 for a, b in edges for v in (a, b) if u[v] in ok)


def test_refuses_a_labeling_message():
    m, u = C.labeling_model()
    _refused(m, None, UNSUPPORTED, "factor %d " % u[1])
    _refused(m, [u[2], u[1]], UNSUPPORTED, "factor %d " % u[1])
    assert E.Plan(m).window_info([u[0], u[2]]) == dict(n_links=2, n_pairwise=2)


def test_labeling_right_factor_is_refused_as_unsupported():
    """the right factor of the labeling message is a VECTOR factor, too: listed, it is refused for its message"""
    m, u = C.labeling_model()
    q = int(np.flatnonzero(m.f_dim0 == 4)[0])
    assert m.f_kind[q] == M.F_VECTOR
    with pytest.raises(E.EngineError) as ei:
        E.Plan(m).window_info([q])
    assert ei.value.code == UNSUPPORTED and "factor %d " % q in str(ei.value)


def test_refuses_duplicate_messages_and_two_unaries_on_one_side():
    m, u, p, edges = C.edge_grid(extra="duplicate")
    i, j = edges[2]
    _refused(m, None, UNSUPPORTED, "factor %d " % u[i])
    _refused(m, [u[i]], UNSUPPORTED, "two messages into one vector")
    assert E.Plan(m).window_info([u[j]])["n_links"] == sum(1 for e in edges if j in e)    # the other side: one unary, one vector
    m, u, p, edges = C.edge_grid(extra="two_unaries")
    i, j = edges[2]
    third = next(int(v) for v in range(9) if v not in (i, j))
    for lst, name in (([u[i]], u[i]), ([u[third]], u[third]), ([u[j]], u[j]), ([u[j], u[third], u[i]], min(u[i], u[j], u[third]))):
        _refused(m, lst, UNSUPPORTED, "factor %d " % name)
    with pytest.raises(E.EngineError) as ei:
        E.Plan(m).window_info([u[i]])
    assert "two different unaries on one side" in str(ei.value)


def test_refuses_bad_lists_naming_the_entry():
    m, u, p, edges = C.edge_grid()
    _refused(m, [u[0], u[3], u[0]], INVALID, "factor %d (entry 2) is listed twice" % u[0])
    _refused(m, [u[0], p[1]], INVALID, "factor %d (entry 1) is not a VECTOR factor" % p[1])
    _refused(m, [u[0], m.n_factors], INVALID, "factor index %d (entry 1) is out of range" % m.n_factors)
    _refused(m, [-1], INVALID, "factor index -1 (entry 0) is out of range")
    # INVALID wins over UNSUPPORTED: the list is checked before the factors
    md, ud, pd, ed = C.edge_grid("dense")
    _refused(md, [ud[ed[4][0]], md.n_factors], INVALID, "out of range")


# ---- the numpy statement -------------------------------------------------------------------------------------------------------
def _after_passes(m, n=2):
    o = Oracle(C.expand(m))
    o.set_reparametrization(M.REPAM_ANISOTROPIC)
    o.ComputePass(n)
    return o.duals()


def test_zero_move_is_the_identity():
    m = C.grid(33, "colour_major")
    d = _after_passes(m)
    m2, d2 = M.move_windows(m, d, None, np.zeros(C.H * C.W, np.int64))
    assert d2.tobytes() == d.tobytes() and m2.const_data.tobytes() == m.const_data.tobytes()
    m3, d3 = M.move_windows(m, d, [], [])
    assert d3.tobytes() == d.tobytes() and m3.const_data.tobytes() == m.const_data.tobytes()
    # equal deltas everywhere: the duals move, no constant is written
    m4, d4 = M.move_windows(m, d, None, np.full(C.H * C.W, 3))
    assert m4.const_data.tobytes() == m.const_data.tobytes() and not np.array_equal(d4, d)


@pytest.mark.parametrize("case", ["grid5", "grid33", "rect", "partial"])
def test_energy_is_invariant_on_labellings_inside_both_windows(case):
    """every labelling whose absolute labels lie in the old and in the new windows has the same reparametrised energy, term by term
    and bit for bit, on the dense expansions of the model before and after the move"""
    if case == "rect":
        m = C.D.rect_chain(dims=(5, 9))
    else:
        m = C.grid(5 if case == "grid5" else 33, "row_major")
    u = C.unaries(m)
    lst = u[::2] if case == "partial" else u[::-1]
    dims = m.f_dim0[lst]
    rng = np.random.default_rng(3)
    d = _after_passes(m)
    tried = 0
    for rep in range(6):
        delta = rng.integers(-(dims // 2), dims // 2 + 1)
        m2, d2 = M.move_windows(m, d, lst, delta)
        xa, xb = C.expand(m), C.expand(m2)
        for _ in range(20):
            lab = C.common_labelling(m, lst, delta, rng)
            assert lab is not None
            ea, eb = C.energy(xa, d, lab[0]), C.energy(xb, d2, lab[1])
            assert ea.tobytes() == eb.tobytes()
            tried += 1
    assert tried == 120
    # a sign error would show: the opposite shift update breaks the invariance
    delta = np.where(np.arange(len(lst)) % 2 == 0, 1, -1)
    m2, d2 = M.move_windows(m, d, lst, delta)
    wrong, _ = M.move_windows(m, d, lst, -delta)
    lab = C.common_labelling(m, lst, delta, rng)
    import dataclasses
    xw = C.expand(dataclasses.replace(m2, const_data=wrong.const_data, _keep=[]))
    assert not np.array_equal(C.energy(C.expand(m), d, lab[0]), C.energy(xw, d2, lab[1]))


def test_shift_saturates_at_2_to_the_30():
    m, u, p, edges = C.edge_grid()
    big = float(M.DIFF_SHIFT_MAX)
    coff = m.const_offsets()
    const = m.const_data.copy()
    e0, e1 = edges.index((0, 1)), edges.index((0, 3))
    const[coff[p[e0]] + 1] = big - 2.0
    const[coff[p[e1]] + 1] = -big + 1.0
    import dataclasses
    m = dataclasses.replace(m, const_data=const, _keep=[])
    d = m.dual_data
    up, _ = M.move_windows(m, d, [u[0]], [5])                 # unary 0 is on side 0 of both edges: shift + 5
    assert up.const_data[coff[p[e0]] + 1] == big and up.const_data[coff[p[e1]] + 1] == -big + 6.0
    down, _ = M.move_windows(m, d, [u[0]], [-5])
    assert down.const_data[coff[p[e0]] + 1] == big - 7.0 and down.const_data[coff[p[e1]] + 1] == -big
    far, _ = M.move_windows(m, d, [u[0], u[1]], [M.MOVE_DELTA_MAX, -M.MOVE_DELTA_MAX])
    assert far.const_data[coff[p[e0]] + 1] == big
    assert np.array_equal(far.const_data[coff[p[e0]]], m.const_data[coff[p[e0]]])          # the scale stays
    with pytest.raises(ValueError):
        M.move_windows(m, d, [u[0]], [M.MOVE_DELTA_MAX + 1])
    with pytest.raises(ValueError):
        M.move_windows(m, d, [u[0]], [0.5])
    with pytest.raises(ValueError):
        M.move_windows(m, d, [u[0]], [1, 2])


def test_cost_rule_equal_and_infinite_entries():
    m = C.grid(5, "row_major")
    u = C.unaries(m)[:6]
    d = _after_passes(m)
    delta = np.array([0, 1, -2, 4, -5, 7])
    off = m.dual_offsets()
    co, cn = C.cost_pair(m, u, delta, 5, stride=9, inf=True)
    assert np.isinf(co).any() and np.isinf(cn).any()
    plain = M.move_windows(m, d, u, delta)[1]
    m2, d2 = M.move_windows(m, d, u, delta, co, cn)
    assert not np.any(np.isnan(d2))
    for i, f in enumerate(u):
        g = np.clip(np.arange(5) + delta[i], 0, 4)
        th, got = d[off[f]:off[f] + 5][g], d2[off[f]:off[f] + 5]
        same = cn[i, :5] == co[i, :5][g]
        assert got[same].tobytes() == th[same].tobytes()                        # equal entries, two +inf included: carried bit for bit
        with np.errstate(invalid="ignore"):
            want = th + (cn[i, :5] - co[i, :5][g])                              # the inner difference first
        assert np.array_equal(got[~same], want[~same])
        assert same.any() if i % 2 == 0 and abs(delta[i]) < 5 else True
    # everything but the listed thetas is what the move without costs gives
    mask = np.ones(d.shape[0], bool)
    for f in u:
        mask[off[f]:off[f] + 5] = False
    assert d2[mask].tobytes() == plain[mask].tobytes() and m2.const_data.tobytes() == M.move_windows(m, d, u, delta)[0].const_data.tobytes()
    with pytest.raises(ValueError):
        M.move_windows(m, d, u, delta, co, None)
    # theta + sum of messages is the original unary: with costs given it becomes the new unary wherever both are finite
    _, links, _ = M.window_links(m, u)
    for i, f in enumerate(u):
        tot = d2[off[f]:off[f] + 5].copy()
        for p, side in links[i]:
            at = off[p] + (5 if side else 0)
            tot += d2[at:at + 5]
        fin = np.isfinite(cn[i, :5])
        assert np.allclose(tot[fin], cn[i, :5][fin], atol=1e-12)


def test_oracle_bound_is_finite_after_a_move():
    for m in (C.grid(33, "colour_major"), C.D.rect_chain(dims=(5, 9))):
        u = C.unaries(m)
        d = _after_passes(m)
        delta = C.deltas(m.f_dim0[u], 4)
        m2, d2 = M.move_windows(m, d, u, delta)
        o = Oracle(C.D.with_duals(C.expand(m2), d2))
        o.set_reparametrization(M.REPAM_ANISOTROPIC)
        lb0 = o.LowerBound()
        o.ComputePass(2)
        assert np.isfinite(lb0) and np.isfinite(o.LowerBound()) and o.LowerBound() >= lb0 - 1e-9


# ---- the LP mirror with the engine stubbed out --------------------------------------------------------------------------------
class StubSet:
    def __init__(self, eng, factors):
        self.eng, self.factors = eng, list(factors)
        self.n = len(self.factors)
        self.max_labels = max(int(eng.model.f_dim0[f]) for f in self.factors)

    def move(self, delta, cost_old=None, cost_new=None):
        self.eng.calls.append(("move", self.factors, np.array(delta), None if cost_old is None else np.array(cost_old),
                               None if cost_new is None else np.array(cost_new)))


class StubEngine:
    def __init__(self):
        self.calls = []

    def upload(self, model, **kw):
        self.model = model; self.calls.append(("upload",))

    def upload_costs(self, const=None, duals=None):
        self.calls.append(("upload_costs",))

    def set_vectors(self, factors, src, accumulate=False):
        self.calls.append(("set_vectors", list(factors)))

    def set_constants(self, factors, src):
        self.calls.append(("set_constants", list(factors)))

    def window_set(self, factors):
        self.calls.append(("window_set", list(factors)))
        return StubSet(self, factors)

    def set_inner_iterations(self, n): pass
    def set_reparametrization_type(self, t): pass
    def set_speculation(self, n): pass


def test_lp_move_windows_keeps_the_books():
    lp, u, p = C.stub_window_lp()
    eng = lp._engine = StubEngine()
    lp.upload_costs()
    assert eng.calls == [("upload",)]
    shifts = [lp.GetFactor(f).shift for f in p]
    costs = [lp.GetFactor(f).cost.copy() for f in u]
    lp.move_windows([u[1], u[2], u[3]], [2, 2, -1])
    assert [c[0] for c in eng.calls[1:]] == ["window_set", "move"] and eng.calls[2][3] is None
    # u0 (unlisted) - u1 (+2): shift - 2;  u1 - u2: equal deltas, untouched;  u2 (+2) - u3 (-1): shift + 3
    assert [lp.GetFactor(f).shift for f in p] == [shifts[0] - 2, shifts[1], shifts[2] + 3]
    for f, dl, c in zip(u, (0, 2, 2, -1), costs):
        assert np.array_equal(lp.GetFactor(f).cost, c[np.clip(np.arange(6) + dl, 0, 5)])
    want = lp.flat_model()
    assert np.array_equal(want.const_data, lp._model.const_data) and np.array_equal(want.dual_data, lp._cost_dual)
    assert not lp._dirty
    n = len(eng.calls)
    lp.upload_costs(warm=True)                    # nothing to send: no constants, no vectors
    assert eng.calls[n:] == []
    # new costs: handed over as the original costs in the old and in the new window; the same set is used again
    new = [np.arange(6.0) + 10 * k for k in range(3)]
    old = [lp.GetFactor(f).cost.copy() for f in u[1:]]
    lp.move_windows([u[1], u[2], u[3]], [0, 1, 0], new_costs=new)
    name, fs, dl, co, cn = eng.calls[-1]
    assert [c[0] for c in eng.calls[n:]] == ["move"] and fs == u[1:] and list(dl) == [0, 1, 0]
    assert np.array_equal(co, np.stack(old)) and np.array_equal(cn, np.stack(new))
    assert [lp.GetFactor(f).shift for f in p] == [shifts[0] - 2, shifts[1] - 1, shifts[2] + 4]
    assert all(np.array_equal(lp.GetFactor(f).cost, c) for f, c in zip(u[1:], new))
    n = len(eng.calls)
    lp.upload_costs(warm=True)
    assert eng.calls[n:] == []
    # a changed cost afterwards is sent as ever
    lp.set_factor_cost(u[0], np.ones(6))
    lp.upload_costs(warm=True)
    assert eng.calls[n:] == [("set_vectors", [u[0]])]
    with pytest.raises(RuntimeError):
        lp.move_windows([u[1]], [1, 2])
    with pytest.raises(RuntimeError):
        lp.move_windows([u[1]], [1], new_costs=[np.zeros(5)])
