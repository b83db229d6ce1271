"""Peer minima with the publish's row reduction as a REDUCE-SCATTER (kernels.hip dense_pq_publish3_body<L, true>,
``chain_dense_pq_scatter_kernel<32, *>``): a publishing record on the column side of a table computes the eight row partials of a
lane first, then three halving exchanges inside the 16-lane row (4, 2 and 1 values move) and one pairing step leave every lane
with ONE row's minimum, and 32 lanes store one entry each, where the all-reduce form ran four DPP steps for each of the eight
rows and had 4 lanes store 8.  ``min`` is exact and every T[a][b] + m'[b] is one rounding of the same operands: the bits are the same.
Every case runs the same calls on the CPU oracle and on three engines created under different switches — the defaults,
``LPMP_PQ_SCATTER=0`` (the all-reduce form, the parent's kernel) and ``LPMP_PQ_HOLD=2`` (two tables in registers): duals
``np.array_equal`` to the oracle and among the engines, the bound within 1e-9 relative, ``factor_lower_bounds()`` within 1e-12 and
every chain launch a peer-minima launch.  The tables are random per edge and never symmetric, so a row stored to another row's
entry shows.  The side-0 RECEIVE keeps the all-reduce form in every kernel; the mixed-side cases run it beside the new publish."""
import re

import numpy as np
import pytest

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from lp_mp_amd import engine as E
from oracle.binding import Oracle

import peer_minima_cases as PC

pytestmark = pytest.mark.gpu

ANISO = M.REPAM_ANISOTROPIC
LB_RTOL = 1e-9                                                # (tests/test_peer_minima_shapes_gpu.py)
NAME = "chain_dense_pk_kernel<32, 2, false, false>"          # the class's name in the timing, whichever form ran
WINDOWS = [(8, 2, 4), (5, 1, 2)]
PASSES = (1, 2, 5, 9, 33)                                     # explicit lists, the periodic template, a slice of 32 + 1
SWITCHES = (("default", None), ("LPMP_PQ_SCATTER=0", ("LPMP_PQ_SCATTER", "0")), ("LPMP_PQ_HOLD=2", ("LPMP_PQ_HOLD", "2")))
GRIDS = [(4, 5), (5, 5), (13, 11)]
MIXED = ["random-flip 13x11", "thinned 13x11", "bipartite 61+45", "stars 3x4"]
LINE = re.compile(r"peer minima launch \(LPMP_PQ_LDS=(\d), LPMP_PQ_WIDE=(\d): (\d+) records per consume ticket, \d+ tickets\): (\d+) resident workgroups per CU, "
                  r"grid (\d+); (\d) tables in registers, (-?\d+) registers, (-?\d+) bytes of scratch; publish: ([a-z-]+)\n")


def _clear(monkeypatch):
    for k in ("LPMP_PQ_HOLD", "LPMP_PQ_LDS", "LPMP_PQ_WIDE", "LPMP_PQ_SCATTER"):
        monkeypatch.delenv(k, raising=False)


def _window(monkeypatch, bands, lag, depth):
    monkeypatch.setenv("LPMP_ROT_BANDS", str(bands)); monkeypatch.setenv("LPMP_ROT_LAG", str(lag)); monkeypatch.setenv("LPMP_ROT_DEPTH", str(depth))


def _grid(H, W):
    return S.grid_model(H, W, 32, order="colour_major", seed=5000 + H * W)


_TRAJECTORY = {}


def _trajectory(key, build):
    """the oracle on a model over PASSES, computed once per model and left unchanged: (duals, bound) after every call and the factors'
    bounds at the end (the window and the order of a launch change nothing in what it computes)"""
    if key not in _TRAJECTORY:
        m = build()
        o = Oracle(m); o.set_reparametrization(ANISO)
        steps = []
        for n in PASSES:
            o.ComputePass(n)
            steps.append((o.duals().copy(), o.LowerBound()))
        flb = np.array([o.factor_lower_bound(f) for f in range(m.n_factors)])
        for d, _ in steps:
            d.setflags(write=False)
        flb.setflags(write=False)
        _TRAJECTORY[key] = (steps, flb)
    return _TRAJECTORY[key]


class Engines:
    """one engine per switch on one model (the switches are read when an engine is created)"""

    def __init__(self, m, monkeypatch):
        self.engines = []
        for _, env in SWITCHES:
            _clear(monkeypatch)
            if env is not None:
                monkeypatch.setenv(*env)
            self.engines.append(E.Engine(0))
        _clear(monkeypatch)
        for e in self.engines:
            e.upload(m); e.set_reparametrization(ANISO)
            assert e.plan.pass_rotates(ANISO) and e.plan.peer_minima(ANISO) == (True, "")

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


def _run(key, build, monkeypatch):
    steps, flb = _trajectory(key, build)
    t = Engines(build(), monkeypatch)
    try:
        for n, (duals, bound) in zip(PASSES, steps):
            t.compute_pass(n, key)
            t.same(duals, bound, (key, n))
        t.same_factor_bounds(flb, key)
    finally:
        t.close()


@pytest.mark.parametrize("bands,lag,depth", WINDOWS)
@pytest.mark.parametrize("H,W", GRIDS)
def test_colour_major_grids(H, W, bands, lag, depth, monkeypatch):
    """every publish is the row reduction (the W records are on the column side of their tables); 5 x 5 leaves dead record slots in the
    last workgroup, 13 x 11 has records with 2, 3 and 4 receives, so the scatter runs on the parked table's slot and on all three others"""
    _window(monkeypatch, bands, lag, depth)
    _run(("grid", H, W), lambda: _grid(H, W), monkeypatch)


@pytest.mark.parametrize("H,W", [(1, 7), (2, 2)])
def test_nothing_parked(H, W, monkeypatch):
    """records with at most two receives: the third slot stays empty"""
    _window(monkeypatch, 8, 2, 4)
    _run(("grid", H, W), lambda: _grid(H, W), monkeypatch)


@pytest.mark.parametrize("bands,lag,depth", WINDOWS)
@pytest.mark.parametrize("name", MIXED)
def test_publishes_on_either_side(name, bands, lag, depth, monkeypatch):
    """publishing records on side 0, on side 1 and on both sides of their tables, with 1-4 edges: the scatter publish beside the column
    publish in one record, and beside the side-0 receive, which keeps the all-reduce form"""
    _window(monkeypatch, bands, lag, depth)
    _run(name, lambda: PC.case(name).model(), monkeypatch)


def _hard(m, L, seed, frac=0.35):
    """+inf entries in the tables; the diagonal stays finite, so every row and column keeps a finite entry (tests/test_peer_minima_gpu.py)"""
    rng = np.random.default_rng(seed)
    T = np.asarray(m.const_data).reshape(-1, L, L)
    mask = rng.random(T.shape) < frac
    mask[:, np.arange(L), np.arange(L)] = False
    T[mask] = np.inf
    return m


def test_hard_constraints(monkeypatch):
    """+inf through the exchanges: a lane's partial of a row may be +inf, the row's minimum stays finite"""
    _window(monkeypatch, 5, 1, 2)
    m = _hard(PC.case("random-flip 13x11").model(), PC.L, 73)
    assert np.isinf(np.asarray(m.const_data)).any()
    o = Oracle(m); o.set_reparametrization(ANISO)
    t = Engines(m, monkeypatch)
    try:
        for n in (1, 3, 9):
            o.ComputePass(n)
            t.compute_pass(n)
            t.same(o.duals(), o.LowerBound(), n, finite=True)
        t.same_factor_bounds(np.array([o.factor_lower_bound(f) for f in range(m.n_factors)]))
    finally:
        t.close()


def test_verbose_line_reports_the_publish_form(monkeypatch, capfd):
    """the default engine reports the reduce-scatter publish, three resident workgroups per CU and no scratch; LPMP_PQ_SCATTER=0 and the
    two-table forms report the all-reduce"""
    monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
    _window(monkeypatch, 8, 2, 4)
    m = _grid(13, 11)
    seen = {}
    for name, env in SWITCHES:
        _clear(monkeypatch)
        if env is not None:
            monkeypatch.setenv(*env)
        e = E.Engine(0)
        try:
            e.upload(m); e.set_reparametrization(ANISO)
            capfd.readouterr()
            e.compute_pass(2)
            found = LINE.findall(capfd.readouterr().err)
            assert found and len(set(found)) == 1, (name, found)
            seen[name] = tuple(int(x) for x in found[0][:-1]) + (found[0][-1],)
        finally:
            e.close()
    lds, wide, per_ticket, per_cu, grid, held, regs, scratch, form = seen["default"]
    assert (lds, wide, per_ticket, held) == (1, 1, 8, 3) and form == "reduce-scatter", seen
    assert per_cu == 3 and scratch == 0 and 0 < regs <= 168, seen
    assert seen["LPMP_PQ_SCATTER=0"][:4] == (1, 1, 8, 3) and seen["LPMP_PQ_SCATTER=0"][5] == 3 and seen["LPMP_PQ_SCATTER=0"][8] == "all-reduce", seen
    assert seen["LPMP_PQ_HOLD=2"][5] == 2 and seen["LPMP_PQ_HOLD=2"][8] == "all-reduce", seen
    for name, v in seen.items():
        assert v[3] == 3 and v[7] == 0, (name, v)
