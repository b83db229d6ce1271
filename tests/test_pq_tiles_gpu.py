"""The ticket order of the peer-minima launches (order.cpp skewed_tile_order, engine.cpp rotation_chain): tiles cut into
sub-bands on one time line, every block at least a gap behind its predecessors.  Only the order of the tickets changes, so every
case runs the same calls on the CPU oracle and on three engines — the skewed tiled order with a small forced geometry, the same
window under ``LPMP_PQ_TILES=0`` (the band order every other launch takes) and under ``LPMP_ROT_TILES=0`` — and asks for duals
``np.array_equal`` to the oracle and among the engines, equal bounds and factor bounds, every chain launch a peer-minima launch, and
a verbose line that names the order that ran.  Grids of 24 x 24, 40 x 24 and 33 x 47, a model with records on either side of their
tables and one with +inf entries; 4, 5, 9, 13 and 33 passes (explicit lists, the periodic template of either tail, a slice of 32 + 1)."""
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
PASSES = (4, 5, 9, 13, 33)
# (tile blocks, sub-bands, lag, gap, depth): the deepest group built is 16 steps
GEOMETRIES = [(3, 3, 1, 1, 8), (6, 3, 2, 1, 4), (4, 1, 1, 0, 2), (5, 3, 2, 2, 16)]
GRIDS = [(24, 24), (40, 24), (33, 47)]
KNOBS = ("LPMP_ROT_BANDS", "LPMP_ROT_LAG", "LPMP_ROT_DEPTH", "LPMP_ROT_TILES", "LPMP_PQ_TILES", "LPMP_PQ_SUB", "LPMP_PQ_SUBLAG", "LPMP_PQ_SUBGAP", "LPMP_PQ_MIN_PASSES")
LAUNCH = re.compile(r"lpmp: \d+ passes as one launch( \([a-z ,]+\))?: \d+ tickets, (\d+) bands, lag (\d+), depth (\d+)")
PQ_LINE = re.compile(r"peer minima launch \(.*?(-?\d+) bytes of scratch")


def _engines(m, geometry, monkeypatch):
    """(name, engine) x 3 on one model; the switches are read when an engine is created"""
    T, sub, lag, gap, depth = geometry
    window = {"LPMP_ROT_BANDS": "8", "LPMP_ROT_LAG": "2", "LPMP_ROT_DEPTH": str(depth)}
    skew = {"LPMP_PQ_SUB": str(sub), "LPMP_PQ_SUBLAG": str(lag), "LPMP_PQ_SUBGAP": str(gap)}
    variants = (("skewed tiles", dict(window, LPMP_ROT_TILES=str(T), **skew)),
                ("LPMP_PQ_TILES=0", dict(window, LPMP_PQ_TILES="0", **skew)),
                ("LPMP_ROT_TILES=0", dict(window, LPMP_ROT_TILES="0", **skew)))
    out = []
    for name, env in variants:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = E.Engine(0)
        e.upload(m); e.set_reparametrization(ANISO)
        assert e.plan.pass_rotates(ANISO) and e.plan.peer_minima(ANISO) == (True, "")
        out.append((name, e))
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return out


_TRAJECTORY = {}


def _trajectory(key, build):
    """the oracle on a model over PASSES, computed once per model and left unchanged"""
    if key not in _TRAJECTORY:
        m = build()
        o = Oracle(m); o.set_reparametrization(ANISO)
        steps = []
        for n in PASSES:
            o.ComputePass(n)
            d = o.duals().copy(); d.setflags(write=False)
            steps.append((d, o.LowerBound()))
        flb = np.array([o.factor_lower_bound(f) for f in range(m.n_factors)])
        flb.setflags(write=False)
        _TRAJECTORY[key] = (steps, flb)
    return _TRAJECTORY[key]


def _run(key, build, geometry, monkeypatch, capfd, finite=False):
    steps, flb = _trajectory(key, build)
    monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
    engines = _engines(build(), geometry, monkeypatch)
    sub, depth = geometry[1], geometry[4]
    try:
        for n, (duals, bound) in zip(PASSES, steps):
            got = []
            for name, e in engines:
                capfd.readouterr()
                e.enable_kernel_timing(True); e.reset_kernel_timing()
                e.compute_pass(n)
                kt = e.kernel_timing(); e.reset_kernel_timing(); e.enable_kernel_timing(False)
                err = capfd.readouterr().err
                (v,) = kt.values()
                assert v["kernel"] == NAME, (name, key, n, kt)
                assert v["chain_launches"] == (n + 31) // 32 and v["peer_minima_launches"] == v["chain_launches"], (name, key, n, kt)
                # the verbose lines of the launches built in this call name the order that ran (a cached launch prints nothing; the
                # first call of an engine builds one)
                launches, pq_lines = LAUNCH.findall(err), PQ_LINE.findall(err)
                if n == PASSES[0]:
                    assert launches and pq_lines, (name, key, n, err)
                for form, bands, _, d in launches:
                    skewed = "skewed tiled order" in form
                    assert skewed == (name == "skewed tiles" and sub > 1), (name, key, n, form)
                    assert ("tiled order" in form) == (name == "skewed tiles"), (name, key, n, form)
                    assert int(d) == depth and int(bands) == 8, (name, key, n, err)
                for scratch in pq_lines:
                    assert int(scratch) == 0, (name, err)
                d = e.download_duals()
                if finite:
                    assert np.isfinite(d).all(), (name, key, n)
                assert np.array_equal(d, duals), (name, "against the oracle", key, n, float(np.max(np.abs(d - duals))))
                lb = e.lower_bound()
                assert abs(lb - bound) <= LB_RTOL * max(1.0, abs(bound)), (name, key, n, lb, bound)
                got.append((d, lb))
            for (name, _), (d, lb) in zip(engines[1:], got[1:]):
                assert np.array_equal(got[0][0], d) and lb == got[0][1], ("skewed tiles against", name, key, n)
        f0 = engines[0][1].factor_lower_bounds()
        assert np.max(np.abs(f0 - flb)) <= 1e-12, key
        for name, e in engines[1:]:
            assert np.array_equal(e.factor_lower_bounds(), f0), (name, key)
    finally:
        for _, e in engines:
            e.close()


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "t%d-s%d-l%d-g%d-d%d" % g)
@pytest.mark.parametrize("H,W", GRIDS)
def test_colour_major_grids(H, W, geometry, monkeypatch, capfd):
    _run(("grid", H, W), lambda: S.grid_model(H, W, 32, order="colour_major", seed=7000 + H * W), geometry, monkeypatch, capfd)


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "t%d-s%d-l%d-g%d-d%d" % g)
def test_records_on_either_side_of_their_tables(geometry, monkeypatch, capfd):
    _run("random-flip 13x11", lambda: PC.case("random-flip 13x11").model(), geometry, monkeypatch, capfd)


def _hard(m, L, seed, frac=0.35):
    """+inf entries in the tables; the diagonal stays finite, so every row and column keeps a finite entry (tests/test_peer_minima_gpu.py)"""
    rng = np.random.default_rng(seed)
    T = np.asarray(m.const_data).reshape(-1, L, L)
    mask = rng.random(T.shape) < frac
    mask[:, np.arange(L), np.arange(L)] = False
    T[mask] = np.inf
    return m


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "t%d-s%d-l%d-g%d-d%d" % g)
def test_hard_constraints(geometry, monkeypatch, capfd):
    def build():
        m = _hard(S.grid_model(24, 24, 32, order="colour_major", seed=7311), 32, 74)
        assert np.isinf(np.asarray(m.const_data)).any()
        return m
    _run("hard 24x24", build, geometry, monkeypatch, capfd, finite=True)


def test_geometry_line_and_the_override(monkeypatch, capfd):
    """the skewed order prints its geometry (tile bytes, depth, sub-bands, lag, delayed shares, predicted HBM share of the table
    reads); under LPMP_PQ_TILES=0 the same engine settings give the band order and no such line"""
    monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
    m = S.grid_model(24, 24, 32, order="colour_major", seed=7576)
    line = re.compile(r"peer-minima geometry: tiles of \d+ MiB of a W step \(\d+ W blocks; steps move [0-9. /]+ GB\), depth (\d+), (\d+) sub-bands per tile at lag (\d+), gap (\d+), "
                      r"delayed after 7 / 11 / 15 steps: [0-9.]+ / [0-9.]+ / [0-9.]+; predicted HBM share of the table reads ([0-9.]+)")
    for name, e in _engines(m, (6, 3, 2, 1, 8), monkeypatch):
        try:
            capfd.readouterr()
            e.compute_pass(9)
            found = line.findall(capfd.readouterr().err)
            if name == "skewed tiles":
                assert found and set(found[0][:4]) <= {"8", "3", "2", "1"} and found[0][:4] == ("8", "3", "2", "1"), found
                assert 0.25 <= float(found[0][4]) <= 1.0, found
            else:
                assert not found, (name, found)
        finally:
            e.close()


def _one(env, m, monkeypatch, **upload):
    """an engine created under exactly these switches"""
    for k in KNOBS + ("LPMP_NO_PEER_MINIMA",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = E.Engine(0)
    e.upload(m, **upload); e.set_reparametrization(ANISO)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return e


def _passes(e, n, capfd):
    """n passes; (forms of the launches built, chain launches, peer-minima launches)"""
    capfd.readouterr()
    e.enable_kernel_timing(True); e.reset_kernel_timing()
    e.compute_pass(n)
    kt = e.kernel_timing(); e.reset_kernel_timing(); e.enable_kernel_timing(False)
    (v,) = kt.values()
    return [f[0] for f in LAUNCH.findall(capfd.readouterr().err)], v["chain_launches"], v["peer_minima_launches"]


def test_launches_that_are_not_peer_minima_keep_the_plain_orders(monkeypatch, capfd):
    """tiles forced with LPMP_ROT_TILES and every sub-band knob set: a peer-minima launch takes the skew; under LPMP_PQ_TILES=0, under
    LPMP_NO_PEER_MINIMA=1 and on float tables the launch names the plain tiled order; the duals are the oracle's (f32: those of the
    band order on the same float tables)"""
    monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
    build = lambda: S.grid_model(24, 24, 32, order="colour_major", seed=7000 + 24 * 24)
    steps, _ = _trajectory(("grid", 24, 24), build)
    tiles = {"LPMP_ROT_BANDS": "8", "LPMP_ROT_LAG": "2", "LPMP_ROT_DEPTH": "8", "LPMP_ROT_TILES": "4",
             "LPMP_PQ_SUB": "3", "LPMP_PQ_SUBLAG": "2", "LPMP_PQ_SUBGAP": "1"}
    bands = dict(tiles, LPMP_ROT_TILES="0")
    m = build()
    engines = [("skewed", _one(tiles, m, monkeypatch), " (skewed tiled order)", True),
               ("LPMP_PQ_TILES=0", _one(dict(tiles, LPMP_PQ_TILES="0"), m, monkeypatch), " (tiled order)", True),
               ("LPMP_NO_PEER_MINIMA=1", _one(dict(tiles, LPMP_NO_PEER_MINIMA="1"), m, monkeypatch), " (tiled order)", False),
               ("f32 tables", _one(tiles, m, monkeypatch, table_precision="f32_round"), " (tiled order)", False),
               ("f32 tables, band order", _one(bands, m, monkeypatch, table_precision="f32_round"), "", False)]
    try:
        duals = {}
        for name, e, form, pq in engines:
            forms, chains, pq_launches = _passes(e, PASSES[0], capfd)
            assert forms and set(forms) == {form}, (name, forms)
            assert chains == 1 and pq_launches == (1 if pq else 0), (name, chains, pq_launches)
            forms, chains, pq_launches = _passes(e, PASSES[1], capfd)
            assert forms and set(forms) == {form} and chains == 1 and pq_launches == (1 if pq else 0), (name, forms, chains, pq_launches)
            duals[name] = e.download_duals()
        for name in ("skewed", "LPMP_PQ_TILES=0", "LPMP_NO_PEER_MINIMA=1"):
            assert np.array_equal(duals[name], steps[1][0]), (name, "against the oracle")
        assert np.array_equal(duals["f32 tables"], duals["f32 tables, band order"])
        assert not np.array_equal(duals["f32 tables"], duals["skewed"])          # (the float tables are other tables)
    finally:
        for _, e, _, _ in engines:
            e.close()


def test_the_rule_itself_at_test_size(monkeypatch, capfd):
    """LPMP_PQ_TILES=T lets the engine's own rule run under a forced band count, here with LPMP_PQ_MIN_PASSES=4: calls of at least 4
    passes take tiles of T blocks at the depth make_tiles gives them and the skew; shorter calls, and every call under
    LPMP_PQ_TILES=0, the band order"""
    monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
    build = lambda: S.grid_model(24, 24, 32, order="colour_major", seed=7000 + 24 * 24)
    steps, _ = _trajectory(("grid", 24, 24), build)
    window = {"LPMP_ROT_BANDS": "8", "LPMP_ROT_LAG": "2", "LPMP_PQ_SUB": "3", "LPMP_PQ_SUBLAG": "2", "LPMP_PQ_SUBGAP": "2"}
    m = build()
    rule, off = _one(dict(window, LPMP_PQ_TILES="4", LPMP_PQ_MIN_PASSES="4"), m, monkeypatch), _one(dict(window, LPMP_PQ_TILES="0"), m, monkeypatch)
    try:
        for n, (duals, _) in zip(PASSES[:3], steps):                     # 4, 5 and 9 passes: explicit lists and the periodic template
            forms, chains, pq_launches = _passes(rule, n, capfd)
            assert forms and all("skewed tiled order" in f for f in forms) and chains == pq_launches == 1, (n, forms)
            forms, chains, pq_launches = _passes(off, n, capfd)
            assert forms and not any("tiled" in f for f in forms) and chains == pq_launches == 1, (n, forms)
            assert np.array_equal(rule.download_duals(), duals) and np.array_equal(off.download_duals(), duals), n
        a, b = rule.download_duals(), off.download_duals()
        forms, chains, pq_launches = _passes(rule, 3, capfd)            # fewer than 4 passes: the old order
        assert forms and not any("tiled" in f for f in forms) and chains == pq_launches == 1, forms
        _passes(off, 3, capfd)
        assert np.array_equal(rule.download_duals(), off.download_duals()) and not np.array_equal(a, rule.download_duals()) and np.array_equal(a, b)
    finally:
        rule.close(); off.close()


def test_short_and_long_calls_on_one_engine_at_the_shipped_threshold(monkeypatch, capfd):
    """the threshold as shipped (12 passes): calls of 8 to 11 passes are periodic templates in the old order, longer ones periodic
    templates in the new one, with the same tails — each finds its own template whatever came before: 20 then 8 passes, 8 then
    20, and 40 (32 + 8) and 42 (32 + 10) passes in one call; duals against the oracle, the order named in the verbose line"""
    monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
    build = lambda: S.grid_model(24, 24, 32, order="colour_major", seed=7000 + 24 * 24)
    o = Oracle(build()); o.set_reparametrization(ANISO)
    after = {}
    done = 0
    for total in (8, 20, 28, 40, 42):
        o.ComputePass(total - done); done = total
        after[total] = o.duals().copy()
    env = {"LPMP_ROT_BANDS": "8", "LPMP_ROT_LAG": "2", "LPMP_PQ_TILES": "4", "LPMP_PQ_SUB": "3", "LPMP_PQ_SUBLAG": "2", "LPMP_PQ_SUBGAP": "2"}
    OLD, NEW = " (periodic template)", " (periodic template, skewed tiled order)"
    # (calls, the forms each call builds)
    for calls in (((20, {NEW}), (8, {OLD})), ((8, {OLD}), (20, {NEW})), ((40, {NEW, OLD}),), ((42, {NEW, OLD}),)):
        e = _one(env, build(), monkeypatch)
        try:
            total = 0
            for n, want in calls:
                forms, chains, pq_launches = _passes(e, n, capfd)
                total += n
                assert set(forms) == want, (calls, n, forms)
                assert chains == pq_launches == (n + 31) // 32, (calls, n, chains, pq_launches)
                assert np.array_equal(e.download_duals(), after[total]), (calls, n)
            n = calls[0][0]                                             # once more: both templates are cached now, nothing is built
            forms, chains, pq_launches = _passes(e, n, capfd)
            assert not forms and chains == pq_launches == (n + 31) // 32, (calls, forms)
        finally:
            e.close()
