"""Joined passes in the peer-minima form on models beyond the colour-major grid (kernels.hip dense_pq_publish_body and
dense_pq_consume_body; the models: tests/peer_minima_cases.py).  On ``synthetic.grid_model(order="colour_major")`` every publishing (W)
record is on side 1 of all its tables and every consuming (H / K / T) record on side 0; here records of either role sit on side 0, on
side 1 and on both, with 1-4 edges, parallel edges and isolated unaries between them — among them the README's own workflow, a grid
inserted row by row and re-inserted in the suggested order.  Every case runs the same calls on the CPU oracle and on three engines
created under different switches — the defaults (wide consume, first table parked in LDS), ``LPMP_PQ_WIDE=0`` and ``LPMP_PQ_LDS=0``:
duals ``np.array_equal`` to the oracle and among the engines, the bound within 1e-9 relative, ``factor_lower_bounds()`` within 1e-12,
every chain launch of every call a peer-minima launch, and the engines' own report (LPMP_ROT_VERBOSE) names the three forms.
The tables are random per edge and never symmetric: a reduction over the wrong side of one table is the model with that table
transposed, whose duals differ (tests/test_peer_minima_shapes_host.py)."""
import re

import numpy as np
import pytest

from lp_mp_amd import model as M
from lp_mp_amd import engine as E
from oracle.binding import Oracle

import peer_minima_cases as PC

pytestmark = pytest.mark.gpu

ANISO, ANISO2 = M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2
LB_RTOL = 1e-9
WINDOWS = [(8, 2, 4), (5, 1, 2), (16, 2, 3), (3, 4, 7)]
BIG_WINDOWS = [(8, 2, 4), (3, 4, 7)]                          # the 40 x 36 cases: an even depth (periodic template) and an odd one
PASSES = (1, 2, 5, 9, 33)                                     # explicit lists, the periodic template, a slice of 32 + 1
SWITCHES = (("default", None), ("LPMP_PQ_WIDE=0", ("LPMP_PQ_WIDE", "0")), ("LPMP_PQ_LDS=0", ("LPMP_PQ_LDS", "0")))
FORM = re.compile(r"LPMP_PQ_LDS=(\d), LPMP_PQ_WIDE=(\d): (\d+) records per consume ticket")
ALL_FORMS = {("1", "1", "8"), ("1", "0", "4"), ("0", "1", "8")}
NAME = "chain_dense_pk_kernel<32, 2, false, false>"          # the class's name in the timing, whichever form ran


def _window(monkeypatch, bands, lag, depth):
    monkeypatch.setenv("LPMP_ROT_BANDS", str(bands)); monkeypatch.setenv("LPMP_ROT_LAG", str(lag)); monkeypatch.setenv("LPMP_ROT_DEPTH", str(depth))


_TRAJECTORY = {}


def _trajectory(name):
    """the oracle on a case of the list over PASSES in REPAM_ANISOTROPIC, computed once and left unchanged: (duals, bound) after every
    call, and the factors' bounds at the end (the window and the order of a launch change nothing in what it computes)"""
    if name not in _TRAJECTORY:
        m = PC.case(name).model()
        o = Oracle(m); o.set_reparametrization(ANISO)
        steps = []
        for n in PASSES:
            o.ComputePass(n)
            steps.append((o.duals().copy(), o.LowerBound()))
        flb = np.array([o.factor_lower_bound(f) for f in range(m.n_factors)])
        for d, _ in steps:
            d.setflags(write=False)
        flb.setflags(write=False)
        _TRAJECTORY[name] = (steps, flb)
    return _TRAJECTORY[name]


class Engines:
    """one engine per switch on one model (the switches are read when an engine is created)"""

    def __init__(self, m, monkeypatch, mode=ANISO):
        monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
        self.engines = []
        for _, env in SWITCHES:
            monkeypatch.delenv("LPMP_PQ_WIDE", raising=False); monkeypatch.delenv("LPMP_PQ_LDS", raising=False)
            if env is not None:
                monkeypatch.setenv(*env)
            self.engines.append(E.Engine(0))
        monkeypatch.delenv("LPMP_PQ_WIDE", raising=False); monkeypatch.delenv("LPMP_PQ_LDS", raising=False)
        for e in self.engines:
            e.upload(m); e.set_reparametrization(mode)
            assert e.plan.pass_rotates(mode) and e.plan.peer_minima(mode) == (True, "")

    def named(self):
        return [(s[0], e) for s, e in zip(SWITCHES, self.engines)]

    def compute_pass(self, n, what=None):
        """n passes on every engine; every chain launch must have been a peer-minima launch (a fall-back to another form fails here)"""
        for name, e in self.named():
            e.enable_kernel_timing(True); e.reset_kernel_timing()
            e.compute_pass(n)
            kt = e.kernel_timing(); e.reset_kernel_timing(); e.enable_kernel_timing(False)
            (v,) = kt.values()
            assert v["kernel"] == NAME, (name, what, n, kt)
            assert v["chain_launches"] == (n + 31) // 32 and v["peer_minima_launches"] == v["chain_launches"], (name, what, n, kt)

    def same(self, duals, bound, what=None, finite=False):
        got = [e.download_duals() for e in self.engines]
        if finite:
            assert all(np.isfinite(d).all() for d in got), what
        for (name, e), d in zip(self.named(), got):
            assert np.array_equal(d, duals), (name, "against the oracle", what, float(np.max(np.abs(d - duals))))
            lb = e.lower_bound()
            assert abs(lb - bound) <= LB_RTOL * max(1.0, abs(bound)), (name, what, lb, bound)
        for (name, _), d in zip(self.named()[1:], got[1:]):
            assert np.array_equal(got[0], d), ("default against", name, what)

    def same_factor_bounds(self, flb, what=None):
        for name, e in self.named():
            assert np.max(np.abs(e.factor_lower_bounds() - flb)) <= 1e-12, (name, what)

    def close(self):
        for e in self.engines:
            e.close()


def _forms(err):
    return set(FORM.findall(err))


def _bit_parity_params():
    for name in PC.CASE_NAMES:
        for w in (BIG_WINDOWS if name.endswith("40x36") else WINDOWS):
            yield pytest.param(name, *w, id="%s-%d:%d:%d" % ((name.replace(" ", "_"),) + w))


@pytest.mark.parametrize("name,bands,lag,depth", list(_bit_parity_params()))
def test_bit_parity(name, bands, lag, depth, monkeypatch, capfd):
    _window(monkeypatch, bands, lag, depth)
    steps, flb = _trajectory(name)
    t = Engines(PC.case(name).model(), monkeypatch)
    try:
        capfd.readouterr()
        for n, (duals, bound) in zip(PASSES, steps):
            t.compute_pass(n, name)
            t.same(duals, bound, (name, n))
        assert _forms(capfd.readouterr().err) == ALL_FORMS
        t.same_factor_bounds(flb, name)
    finally:
        t.close()


@pytest.mark.parametrize("name", ["suggested 13x11", "random-flip 13x11", "thinned 13x11"])
def test_both_anisotropic_modes(name, monkeypatch, capfd):
    """REPAM_ANISOTROPIC2 joins as well (Plan.peer_minima); a switch to REPAM_ANISOTROPIC and back on the live engines"""
    _window(monkeypatch, 8, 2, 4)
    m = PC.case(name).model()
    o = Oracle(m); o.set_reparametrization(ANISO2)
    t = Engines(m, monkeypatch, ANISO2)
    try:
        capfd.readouterr()
        for mode, n in ((ANISO2, 2), (ANISO2, 9), (ANISO, 5), (ANISO, 9), (ANISO2, 1), (ANISO2, 9)):
            o.set_reparametrization(mode)
            for e in t.engines:
                e.set_reparametrization(mode)
            o.ComputePass(n)
            t.compute_pass(n, (name, mode))
            t.same(o.duals(), o.LowerBound(), (name, mode, n))
        assert _forms(capfd.readouterr().err) == ALL_FORMS
        t.same_factor_bounds(np.array([o.factor_lower_bound(f) for f in range(m.n_factors)]), name)
    finally:
        t.close()


@pytest.mark.parametrize("name", ["suggested 13x11", "suggested 40x36", "random-flip 13x11", "random-flip 40x36"])
def test_tiled_order(name, monkeypatch, capfd):
    _window(monkeypatch, 8, 2, 4)
    monkeypatch.setenv("LPMP_ROT_TILES", "3")
    steps, flb = _trajectory(name)
    t = Engines(PC.case(name).model(), monkeypatch)
    try:
        capfd.readouterr()
        for n, (duals, bound) in zip(PASSES, steps):
            t.compute_pass(n, name)
            t.same(duals, bound, (name, n))
        err = capfd.readouterr().err
        assert "tiled order" in err and _forms(err) == ALL_FORMS
        t.same_factor_bounds(flb, name)
    finally:
        t.close()


def _hard(m, L, seed, frac=0.35):
    """+inf entries in the tables; the diagonal stays finite, so every row and column keeps a finite entry (tests/test_peer_minima_gpu.py)"""
    rng = np.random.default_rng(seed)
    T = np.asarray(m.const_data).reshape(-1, L, L)
    mask = rng.random(T.shape) < frac
    mask[:, np.arange(L), np.arange(L)] = False
    T[mask] = np.inf
    return m


def test_hard_constraints(monkeypatch, capfd):
    _window(monkeypatch, 5, 1, 2)
    m = _hard(PC.case("random-flip 13x11").model(), PC.L, 63)
    assert np.isinf(np.asarray(m.const_data)).any()
    o = Oracle(m); o.set_reparametrization(ANISO)
    t = Engines(m, monkeypatch)
    try:
        capfd.readouterr()
        for n in (1, 3, 9):
            o.ComputePass(n)
            t.compute_pass(n)
            t.same(o.duals(), o.LowerBound(), n, finite=True)
        assert _forms(capfd.readouterr().err) == ALL_FORMS
        t.same_factor_bounds(np.array([o.factor_lower_bound(f) for f in range(m.n_factors)]))
    finally:
        t.close()


def test_per_pass_bound_rows(monkeypatch, capfd):
    """speculative batches: one pass and its bound per call, the passes run ahead as one joined launch with a bound row per seam — the
    HIST_MID stores of the consuming records and the HIST_END stores of the publishing ones, on records of mixed sides.  Every unary of
    the case keeps an edge, so every factor's bound is written by a record of the launch."""
    _window(monkeypatch, 8, 2, 4)
    m = PC.case("thinned 14x10").model()
    o = Oracle(m); o.set_reparametrization(ANISO)
    t = Engines(m, monkeypatch)
    try:
        capfd.readouterr()
        for e in t.engines:
            e.set_speculation(8); e.reset_kernel_timing()          # (timing stays off: a timed engine does not run ahead)
        for k in range(21):
            o.ComputePass(1)
            lbo = o.LowerBound()
            for name, e in t.named():
                e.compute_pass(1)
                lb = e.lower_bound()
                assert abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (name, k, lb, lbo)
        for name, e in t.named():
            st = e.speculation_stats()
            assert st["batches"] > 0 and st["passes_launched"] >= 21, (name, st)
            assert e.peer_minima_launches() >= st["batches"], name
            e.set_speculation(0)
        t.same(o.duals(), o.LowerBound())
        assert _forms(capfd.readouterr().err) == ALL_FORMS
        t.same_factor_bounds(np.array([o.factor_lower_bound(f) for f in range(m.n_factors)]))
    finally:
        t.close()


def _old_form_models():
    c = PC.case("random-flip 14x10")
    E_ = c.edges.shape[0]
    f32 = np.random.default_rng(64).uniform(0, 1, (E_, PC.L, PC.L)).astype(np.float32).astype(np.float64)   # float-valued costs: exact in float storage
    return {
        "switched off": (lambda: c.model(), {"LPMP_NO_PEER_MINIMA": "1"}, None, NAME),
        "float tables": (lambda: c.model(f32), {}, "f32", "chain_dense_pk_f32_kernel<32, 2, false, false>"),
        "16 labels": (lambda: PC.bipartite_model(c.n0, c.n1, c.edges, c.flip, c.side1_first, L=16, seed=65), {}, None, "chain_dense_pk_kernel<16, 2, false, false>"),
    }


@pytest.mark.parametrize("what", ["switched off", "float tables", "16 labels"])
def test_old_joined_forms_on_the_same_models(what, monkeypatch, capfd):
    """the chain forms of dense_pk_body have only run colour-major grids either: the 14 x 10 grid with random flips with the peer
    minima switched off, on float tables and with 16 labels — one joined launch per call, none of them a peer-minima launch"""
    _window(monkeypatch, 8, 2, 4)
    monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
    build, env, precision, kernel = _old_form_models()[what]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = build()
    o = Oracle(m); o.set_reparametrization(ANISO)
    e = E.Engine(0)
    try:
        e.upload(m, table_precision=precision); e.set_reparametrization(ANISO)
        assert e.table_precision() == (precision or "f64")
        capfd.readouterr()
        for n in (2, 9):
            e.enable_kernel_timing(True); e.reset_kernel_timing()
            e.compute_pass(n); o.ComputePass(n)
            kt = e.kernel_timing(); e.reset_kernel_timing(); e.enable_kernel_timing(False)
            assert [v["kernel"] for v in kt.values()] == [kernel], (what, kt)
            assert all(v["chain_launches"] == 1 and v.get("peer_minima_launches", 0) == 0 for v in kt.values()), (what, kt)
            d, do = e.download_duals(), o.duals()
            assert np.array_equal(d, do), (what, n, float(np.max(np.abs(d - do))))
            lb, lbo = e.lower_bound(), o.LowerBound()
            assert abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (what, n, lb, lbo)
        assert e.peer_minima_launches() == 0 and not _forms(capfd.readouterr().err)
    finally:
        e.close()
