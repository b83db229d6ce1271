"""Peer-minima tickets that start from a descriptor (kernels.hip chain_loop_roles_ahead, ``chain_dense_pq_ahead_kernel``):
the next ticket's descriptor — launch, block, dependency count, the first predecessors inline — is fetched by wave 0 during the
current body, the call's launch table lives in LDS, and a ticket issues the first poll of its predecessors' flags right behind its
packet request.  Only WHEN a ticket learns what it is changes, so every case runs the same calls on the CPU oracle and on engines
created under different switches — the default (tickets ahead) and ``LPMP_PQ_AHEAD=0`` (the kernel and tables without descriptors) at
least — and asks for duals ``np.array_equal`` to the oracle and among the engines, bounds and factor bounds equal (``==``) among the
engines.  Against the ORACLE the bounds are compared to 1e-9 relative and the factor bounds to 1e-12 absolute, also in the speculation
case: this departs from the issue's word "equal" — the engine sums the factors' bounds in another order than the CPU oracle, in the
parent as in this tree, so bit equality to the oracle was never a property of the bound (the tolerances are those of
tests/test_peer_minima_hold_gpu.py and tests/test_pq_tiles_gpu.py; the duals, which the bound is a sum over, ARE bit-equal).  Every chain
launch a peer-minima launch, and verbose lines that name the form, 0 bytes of scratch and three workgroups per CU.
32 labels, dense f64 tables, colour-major order throughout.  Shapes: 2 x 2, 3 x 3 and 5 x 7 (records with 2 and 3 receives, last
tickets that are not full); 12 x 12 on 1, 2 and 8 workgroups (``LPMP_CHAIN_MAX_WGS``: dozens of tickets in a row per workgroup, so
the descriptor rotation and the guard at the last ticket run deterministically); 24 x 24 in the skewed tiled order at 33 and 40
passes, 20 + 8 and 8 + 20 (periodic template, flag ring); inline caps 0 and 1 (every ticket through dep[]); records on either
side of their tables; +inf entries; speculative single-pass calls (the bound row of a copy from the descriptor); ``LPMP_PQ_WIDE=0``
and ``LPMP_PQ_HOLD=2``, which keep the plain loop and say so."""
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
KNOBS = ("LPMP_ROT_BANDS", "LPMP_ROT_LAG", "LPMP_ROT_DEPTH", "LPMP_ROT_TILES", "LPMP_PQ_TILES", "LPMP_PQ_SUB", "LPMP_PQ_SUBLAG", "LPMP_PQ_SUBGAP",
         "LPMP_PQ_MIN_PASSES", "LPMP_PQ_AHEAD", "LPMP_PQ_DESC_INLINE", "LPMP_CHAIN_MAX_WGS", "LPMP_PQ_WIDE", "LPMP_PQ_HOLD", "LPMP_PQ_LDS", "LPMP_PQ_SCATTER")
WINDOW = {"LPMP_ROT_BANDS": "8", "LPMP_ROT_LAG": "2", "LPMP_ROT_DEPTH": "4"}
# the skewed tiled order at test size (tests/test_pq_tiles_gpu.py, the shipped threshold of 12 passes)
SKEW = {"LPMP_ROT_BANDS": "8", "LPMP_ROT_LAG": "2", "LPMP_PQ_TILES": "4", "LPMP_PQ_SUB": "3", "LPMP_PQ_SUBLAG": "2", "LPMP_PQ_SUBGAP": "2"}
# the launch's line and, right behind it, the line that names the ticket form
PQ_LINE = re.compile(r"peer minima launch \(.*?(\d+) resident workgroups per CU, grid (\d+); (\d) tables in registers, (-?\d+) registers, (-?\d+) bytes of scratch; "
                     r"publish: ([a-z-]+)\nlpmp:   peer minima launch; tickets: (ahead|plain)")
AHEAD, PLAIN = ("ahead", {}), ("LPMP_PQ_AHEAD=0", {"LPMP_PQ_AHEAD": "0"})


def _grid(H, W):
    return S.grid_model(H, W, 32, order="colour_major", seed=9100 + H * W)


def _hard(m, L, seed, frac=0.35):
    """+inf entries in the tables; the diagonal stays finite (tests/test_pq_tiles_gpu.py)"""
    rng = np.random.default_rng(seed)
    T = np.asarray(m.const_data).reshape(-1, L, L)
    mask = rng.random(T.shape) < frac
    mask[:, np.arange(L), np.arange(L)] = False
    T[mask] = np.inf
    return m


MODELS = {
    "2x2": lambda: _grid(2, 2), "3x3": lambda: _grid(3, 3), "5x7": lambda: _grid(5, 7), "12x12": lambda: _grid(12, 12), "24x24": lambda: _grid(24, 24),
    "random-flip 13x11": lambda: PC.case("random-flip 13x11").model(),
    "hard 24x24": lambda: _hard(_grid(24, 24), 32, 91),
}
_TRAJECTORY = {}


def _trajectory(key, calls):
    """the oracle on a model over a sequence of calls, computed once and left unchanged: (duals, bound) after every call, and the
    factors' bounds at the end"""
    if (key, calls) not in _TRAJECTORY:
        m = MODELS[key]()
        o = Oracle(m); o.set_reparametrization(ANISO)
        steps = []
        for n in calls:
            o.ComputePass(n)
            d = o.duals().copy(); d.setflags(write=False)
            steps.append((d, o.LowerBound()))
        flb = np.array([o.factor_lower_bound(f) for f in range(m.n_factors)])
        flb.setflags(write=False)
        _TRAJECTORY[(key, calls)] = (steps, flb)
    return _TRAJECTORY[(key, calls)]


def _engine(m, env, monkeypatch):
    """an engine created under exactly these switches (they are read when an engine is created)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = E.Engine(0)
    e.upload(m); e.set_reparametrization(ANISO)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    assert e.plan.pass_rotates(ANISO) and e.plan.peer_minima(ANISO) == (True, "")
    return e


def _run(key, calls, variants, common, monkeypatch, capfd, finite=False, max_grid=None):
    """variants: (name, env, tickets the verbose line must name); common: switches of every engine; max_grid: what the grid the
    verbose line reports may not exceed (LPMP_CHAIN_MAX_WGS)"""
    steps, flb = _trajectory(key, tuple(calls))
    monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
    m = MODELS[key]()
    engines = [(name, _engine(m, dict(common, **env), monkeypatch), tickets) for name, env, tickets in variants]
    try:
        seen = {name: [] for name, _, _ in engines}
        for n, (duals, bound) in zip(calls, steps):
            got = []
            for name, e, tickets in engines:
                capfd.readouterr()
                e.enable_kernel_timing(True); e.reset_kernel_timing()
                e.compute_pass(n)
                kt = e.kernel_timing(); e.reset_kernel_timing(); e.enable_kernel_timing(False)
                err = capfd.readouterr().err
                (v,) = kt.values()
                assert v["kernel"] == NAME, (name, key, n, kt)
                assert v["chain_launches"] == (n + 31) // 32 and v["peer_minima_launches"] == v["chain_launches"], (name, key, n, kt)
                for per_cu, grid, held, regs, scratch, publish, form in PQ_LINE.findall(err):
                    print(key, name, n, "passes:", per_cu, "per CU, grid", grid, held, "tables,", regs, "registers,", scratch, "bytes of scratch,", publish, form)
                    assert form == tickets and int(scratch) == 0 and int(per_cu) == 3, (name, key, n, err)
                    assert max_grid is None or 1 <= int(grid) <= max_grid, (name, key, n, grid, max_grid)
                    seen[name].append(form)
                d = e.download_duals()
                if finite:
                    assert np.isfinite(d).all(), (name, key, n)
                assert np.array_equal(d, duals), (name, "against the oracle", key, n, float(np.max(np.abs(d - duals))))
                lb = e.lower_bound()
                assert abs(lb - bound) <= LB_RTOL * max(1.0, abs(bound)), (name, key, n, lb, bound)
                got.append((d, lb))
            for (name, _, _), (d, lb) in zip(engines[1:], got[1:]):
                assert np.array_equal(got[0][0], d) and lb == got[0][1], (engines[0][0], "against", name, key, n)
        for name, _, _ in engines:
            assert seen[name], (name, key, "no verbose line of a peer-minima launch")
        f0 = engines[0][1].factor_lower_bounds()
        assert np.max(np.abs(f0 - flb)) <= 1e-12, key
        for name, e, _ in engines[1:]:
            assert np.array_equal(e.factor_lower_bounds(), f0), (name, key)
    finally:
        for _, e, _ in engines:
            e.close()


def _both(extra=None):
    extra = extra or {}
    return [(AHEAD[0], dict(AHEAD[1], **extra), "ahead"), (PLAIN[0], dict(PLAIN[1], **extra), "plain")]


@pytest.mark.parametrize("key", ["2x2", "3x3", "5x7"])
def test_tiny_grids(key, monkeypatch, capfd):
    """records with 2 and 3 receives; blocks whose last ticket holds fewer than 4 W records or 8 consume records"""
    _run(key, (1, 2, 5, 9), _both(), WINDOW, monkeypatch, capfd)


@pytest.mark.parametrize("wgs", [1, 2, 8])
def test_few_workgroups_take_many_tickets_each(wgs, monkeypatch, capfd):
    """the grid is capped (the verbose line's grid is at most LPMP_CHAIN_MAX_WGS), so each workgroup takes many tickets in a row"""
    _run("12x12", (5, 33), _both({"LPMP_CHAIN_MAX_WGS": str(wgs)}), WINDOW, monkeypatch, capfd, max_grid=wgs)


@pytest.mark.parametrize("calls", [(33,), (40,), (20, 8), (8, 20)], ids=lambda c: "+".join(map(str, c)))
def test_periodic_template_and_flag_ring_in_the_skewed_tiled_order(calls, monkeypatch, capfd):
    _run("24x24", calls, _both(), SKEW, monkeypatch, capfd)


@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("key,common,calls", [("12x12", WINDOW, (5, 9)), ("24x24", SKEW, (5, 20))], ids=["12x12", "24x24"])
def test_every_ticket_through_the_overflow_path(key, common, calls, cap, monkeypatch, capfd):
    _run(key, calls, _both() + [("inline cap %d" % cap, {"LPMP_PQ_DESC_INLINE": str(cap)}, "ahead")], common, monkeypatch, capfd)


def test_records_on_either_side_of_their_tables(monkeypatch, capfd):
    _run("random-flip 13x11", (1, 5, 13), _both(), WINDOW, monkeypatch, capfd)


def test_hard_constraints(monkeypatch, capfd):
    assert np.isinf(np.asarray(MODELS["hard 24x24"]().const_data)).any()
    _run("hard 24x24", (5, 20), _both(), SKEW, monkeypatch, capfd, finite=True)


def test_forms_without_the_new_loop_say_so(monkeypatch, capfd):
    """LPMP_PQ_WIDE=0 and LPMP_PQ_HOLD=2 keep the plain loop (their kernels are the shipped ones) beside the default"""
    _run("24x24", (5, 20), [("default", {}, "ahead"), ("LPMP_PQ_WIDE=0", {"LPMP_PQ_WIDE": "0"}, "plain"), ("LPMP_PQ_HOLD=2", {"LPMP_PQ_HOLD": "2"}, "plain")],
         SKEW, monkeypatch, capfd)


def test_per_pass_bounds_of_speculative_batches(monkeypatch):
    """12 single-pass calls with speculation on: the passes run ahead as joined launches with one bound row per seam, the row of a
    copy of the period computed from the descriptor's launch; every pass's bound is the oracle's"""
    m = MODELS["24x24"]()
    o = Oracle(MODELS["24x24"]()); o.set_reparametrization(ANISO)
    engines = [(name, _engine(m, dict(SKEW, **env), monkeypatch)) for name, env in (AHEAD, PLAIN)]
    try:
        for _, e in engines:
            e.set_speculation(8); e.reset_kernel_timing()          # (timing stays off: a timed engine does not run ahead)
        for k in range(12):
            o.ComputePass(1)
            lbo = o.LowerBound()
            lbs = []
            for name, e in engines:
                e.compute_pass(1)
                lbs.append(e.lower_bound())
                assert abs(lbs[-1] - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (name, k, lbs[-1], lbo)
            assert lbs[0] == lbs[1], (k, lbs)
        for name, e in engines:
            st = e.speculation_stats()
            assert st["batches"] > 0 and st["passes_launched"] >= 12, (name, st)
            assert e.peer_minima_launches() >= st["batches"], name
            e.set_speculation(0)
            assert np.array_equal(e.download_duals(), o.duals()), name
    finally:
        for _, e in engines:
            e.close()
