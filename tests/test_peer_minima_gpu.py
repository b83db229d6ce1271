"""Joined passes in the peer-minima form (kernels.hip dense_pq_*_body): the W records of H, W, (K, W)^(n-1), T publish
per edge the minima the record at the other end would compute from the table, and the H / K / T records read no table.  Every case:
32 labels (unless it is a fall-back case), dense tables, anisotropic weights, duals ``np.array_equal`` to the CPU oracle, the bound within
1e-9 relative, and ``peer_minima_launches`` says which form ran."""
import dataclasses

import numpy as np
import pytest

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from lp_mp_amd import engine as E
from oracle.binding import Oracle

pytestmark = pytest.mark.gpu

ANISO = M.REPAM_ANISOTROPIC
LB_RTOL = 1e-9
WINDOWS = [(8, 2, 4), (5, 1, 2), (16, 2, 3), (3, 4, 7)]
GRIDS = [(2, 2), (1, 7), (3, 3), (13, 11), (14, 10), (40, 36)]
OLD_NAME = "chain_dense_pk_kernel<32, 2, false, false>"


def _window(monkeypatch, bands, lag, depth):
    monkeypatch.setenv("LPMP_ROT_BANDS", str(bands)); monkeypatch.setenv("LPMP_ROT_LAG", str(lag)); monkeypatch.setenv("LPMP_ROT_DEPTH", str(depth))


def _timed_pass(e, o, n):
    """n passes on both; returns the engine's timing entries of the call"""
    e.enable_kernel_timing(True); e.reset_kernel_timing()
    e.compute_pass(n); o.ComputePass(n)
    kt = e.kernel_timing(); e.reset_kernel_timing(); e.enable_kernel_timing(False)
    return kt


def _same(e, o, what=None):
    d, do = e.download_duals(), o.duals()
    assert np.array_equal(d, do), (what, float(np.max(np.abs(d - do))))
    lb, lbo = e.lower_bound(), o.LowerBound()
    assert abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (what, lb, lbo)


def _new_form(kt, n, what=None):
    (v,) = kt.values()
    assert v["kernel"] == OLD_NAME, (what, kt)                        # the class's name, whichever form ran
    assert v["chain_launches"] == (n + 31) // 32 and v["peer_minima_launches"] == v["chain_launches"], (what, kt)


def _old_form(kt, what=None):
    for v in kt.values():
        assert v.get("peer_minima_launches", 0) == 0, (what, kt)


@pytest.mark.parametrize("H,W", GRIDS)
@pytest.mark.parametrize("bands,lag,depth", WINDOWS)
def test_bit_parity_on_small_grids(H, W, bands, lag, depth, monkeypatch):
    """border records have 1-3 edges; the pass counts take explicit lists, the periodic template and slices of 32 + 32 + 6"""
    _window(monkeypatch, bands, lag, depth)
    m = S.grid_model(H, W, 32, order="colour_major", seed=H * W + bands)
    o = Oracle(m); o.set_reparametrization(ANISO)
    e = E.Engine(0)
    try:
        e.upload(m); e.set_reparametrization(ANISO)
        assert e.plan.pass_rotates(ANISO)
        for n in (1, 2, 5, 9, 20, 33, 70):
            kt = _timed_pass(e, o, n)
            _new_form(kt, n, (H, W, n))
            _same(e, o, (H, W, n))
        flb = e.factor_lower_bounds()
        assert np.max(np.abs(flb - np.array([o.factor_lower_bound(f) for f in range(m.n_factors)]))) <= 1e-12
    finally:
        e.close()


@pytest.mark.parametrize("H,W", [(13, 11), (40, 36)])
def test_tiled_order(H, W, monkeypatch):
    _window(monkeypatch, 8, 2, 4)
    monkeypatch.setenv("LPMP_ROT_TILES", "3")
    m = S.grid_model(H, W, 32, order="colour_major", seed=77)
    o = Oracle(m); o.set_reparametrization(ANISO)
    e = E.Engine(0)
    try:
        e.upload(m); e.set_reparametrization(ANISO)
        for n in (1, 2, 5, 9, 20, 33):
            _new_form(_timed_pass(e, o, n), n, n)
            _same(e, o, n)
    finally:
        e.close()


def _hard(m, L, seed, frac=0.35):
    """+inf entries in the tables; the diagonal stays finite, so every row and column keeps a finite entry (tests/test_round6_gpu.py)"""
    rng = np.random.default_rng(seed)
    T = np.asarray(m.const_data).reshape(-1, L, L)
    mask = rng.random(T.shape) < frac
    mask[:, np.arange(L), np.arange(L)] = False
    T[mask] = np.inf
    return m


def test_hard_constraints(monkeypatch):
    _window(monkeypatch, 5, 1, 2)
    m = _hard(S.grid_model(13, 11, 32, order="colour_major", seed=61), 32, 61)
    o = Oracle(m); o.set_reparametrization(ANISO)
    e = E.Engine(0)
    try:
        e.upload(m); e.set_reparametrization(ANISO)
        for n in (1, 3, 9):
            _new_form(_timed_pass(e, o, n), n, n)
            assert np.isfinite(e.download_duals()).all()
            _same(e, o, n)
    finally:
        e.close()


def test_per_pass_bound_rows(monkeypatch):
    """speculative batches: one pass and its bound per call, the passes run ahead as one joined launch with a bound row per seam"""
    _window(monkeypatch, 8, 2, 4)
    m = S.grid_model(14, 10, 32, order="colour_major", seed=9)
    o = Oracle(m); o.set_reparametrization(ANISO)
    e = E.Engine(0)
    try:
        e.upload(m); e.set_reparametrization(ANISO)
        e.set_speculation(8)
        e.reset_kernel_timing()                      # (timing stays off: a timed engine does not run ahead)
        for k in range(21):
            e.compute_pass(1); o.ComputePass(1)
            lb, lbo = e.lower_bound(), o.LowerBound()
            assert abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (k, lb, lbo)
        st = e.speculation_stats()
        assert st["batches"] > 0 and st["passes_launched"] >= 21, st
        assert e.peer_minima_launches() >= st["batches"]
        e.set_speculation(0)
        _same(e, o)
    finally:
        e.close()


def _oracle_with(m, duals, mode=ANISO):
    o = Oracle(m); o.set_reparametrization(mode); o.set_duals(duals)
    return o


@pytest.mark.parametrize("what", ["upload_costs", "set_constants", "upload_duals", "mode_switch"])
def test_nothing_published_is_read_across_calls(what, monkeypatch):
    """the published minima of a call are never read by the next one (every call starts with H + W): new tables, new constants of a few
    factors, other duals and another weight mode in between need no invalidation"""
    _window(monkeypatch, 8, 2, 4)
    L = 32
    m = S.grid_model(13, 11, L, order="colour_major", seed=3)
    o = Oracle(m); o.set_reparametrization(ANISO)
    e = E.Engine(0)
    try:
        e.upload(m); e.set_reparametrization(ANISO)
        _new_form(_timed_pass(e, o, 3), 3)
        _same(e, o, "before")
        built = e.schedules_built()
        if what == "upload_costs":
            const = 0.25 + S.u01(np.asarray(m.const_data).shape[0], 991)
            e.upload_costs(const=const)
            o = _oracle_with(dataclasses.replace(m, const_data=const, _keep=[]), o.duals())
        elif what == "set_constants":
            pw = np.flatnonzero(np.asarray(m.f_kind) != M.F_VECTOR)[[0, 5, 17, 40, -1]].astype(np.int32)
            rows = 0.5 + S.u01(pw.shape[0] * L * L, 992).reshape(pw.shape[0], L * L)
            e.set_constants(pw, rows)
            const = np.array(m.const_data, np.float64, copy=True)
            coff = m.const_offsets()
            for i, f in enumerate(pw):
                const[coff[f]:coff[f] + L * L] = rows[i]
            o = _oracle_with(dataclasses.replace(m, const_data=const, _keep=[]), o.duals())
        elif what == "upload_duals":
            d = o.duals() + (S.u01(o.duals().shape[0], 993) - 0.5)
            e.upload_duals(d); o.set_duals(d)
        else:
            e.set_reparametrization(M.REPAM_UNIFORM); o.set_reparametrization(M.REPAM_UNIFORM)
            e.compute_pass(2); o.ComputePass(2)
            _same(e, o, "other mode")
            e.set_reparametrization(ANISO); o.set_reparametrization(ANISO)
        if what in ("upload_costs", "set_constants"):
            assert e.schedules_built() == built
        _new_form(_timed_pass(e, o, 4), 4)
        _same(e, o, what)
    finally:
        e.close()


def test_switch_off(monkeypatch):
    _window(monkeypatch, 8, 2, 4)
    monkeypatch.setenv("LPMP_NO_PEER_MINIMA", "1")
    m = S.grid_model(14, 10, 32, order="colour_major", seed=12)
    o = Oracle(m); o.set_reparametrization(ANISO)
    e = E.Engine(0)
    try:
        e.upload(m); e.set_reparametrization(ANISO)
        for n in (2, 9):
            kt = _timed_pass(e, o, n)
            (v,) = kt.values()
            assert v["kernel"] == OLD_NAME and v["chain_launches"] == 1 and v["peer_minima_launches"] == 0, kt
            _same(e, o, n)
    finally:
        e.close()


def star_model(L=32, leaves=5, arms=3, seed=5):
    """a bipartite graph in a 2-colour order: `arms` centres (colour 1) with `leaves` leaves (colour 0) each — degree 5 > 4 edges"""
    rng = np.random.default_rng(seed)
    b = M.ModelBuilder(2, S.mrf_mtypes())
    leaf = [[b.add_vector_factors(0, rng.uniform(0, 1, (1, L)))[0] for _ in range(leaves)] for _ in range(arms)]
    pw = [[b.add_dense_pairwise(1, rng.uniform(0, 1, (1, L, L)))[0] for _ in range(leaves)] for _ in range(arms)]
    centre = [b.add_vector_factors(0, rng.uniform(0, 1, (1, L)))[0] for _ in range(arms)]
    for a in range(arms):
        for i in range(leaves):
            b.add_messages(0, leaf[a][i], pw[a][i]); b.add_messages(1, centre[a], pw[a][i])
            b.add_relations(leaf[a][i], pw[a][i]); b.add_relations(pw[a][i], centre[a])
    return b.finish()


def _fallback(m, monkeypatch, rtype=0, f32=False, rows=False):
    _window(monkeypatch, 8, 2, 4)
    o = Oracle(m); o.set_reparametrization(ANISO)
    e = E.Engine(0)
    try:
        e.upload(m, rows_layout=True if rows else None, table_precision="f32" if f32 else None); e.set_reparametrization(ANISO)
        assert bool(e.rows_layout) == rows and e.table_precision() == ("f32" if f32 else "f64")
        if rtype:
            e.set_reparametrization_type(rtype); o.set_reparametrization_type(rtype)
        kts = []
        for n in (2, 5):
            kt = _timed_pass(e, o, n)
            _old_form(kt, n)
            _same(e, o, n)
            kts.append(kt)
        return kts
    finally:
        e.close()


def test_fall_back_degree_five(monkeypatch):
    for kt in _fallback(star_model(), monkeypatch):
        assert all(v["kernel"] == OLD_NAME for v in kt.values()) or not any(v.get("chain_launches") for v in kt.values()), kt


@pytest.mark.parametrize("L,name", [(21, "chain_dense_pk_kernel<32, 2, true, false>"), (16, "chain_dense_pk_kernel<16, 2, false, false>")])
def test_fall_back_other_label_counts(L, name, monkeypatch):
    for kt in _fallback(S.grid_model(14, 10, L, order="colour_major", seed=L), monkeypatch):
        assert [v["kernel"] for v in kt.values()] == [name] and all(v["chain_launches"] == 1 for v in kt.values()), kt


def test_fall_back_float_tables(monkeypatch):
    m = S.grid_model(14, 10, 32, order="colour_major", seed=8)
    c = np.asarray(m.const_data); c[:] = c.astype(np.float32)                   # float-valued costs: exact in float storage
    for kt in _fallback(m, monkeypatch, f32=True):
        assert [v["kernel"] for v in kt.values()] == ["chain_dense_pk_f32_kernel<32, 2, false, false>"], kt


def test_fall_back_residual_send_rule(monkeypatch):
    for kt in _fallback(S.grid_model(14, 10, 32, order="colour_major", seed=8), monkeypatch, rtype=1):
        assert not any(v.get("chain_launches") for v in kt.values()), kt        # (no joined launch under that rule at all)


def test_fall_back_rows_layout(monkeypatch):
    _fallback(S.grid_model(14, 10, 32, order="colour_major", seed=8), monkeypatch, rows=True)


def test_medium_size_without_override():
    """384 x 384 (2.4 GB of tables, above the engine's 1 GiB threshold): the engine's own choice is the new form"""
    m = S.grid_model(384, 384, 32, order="colour_major", seed=5)
    o = Oracle(m); o.set_reparametrization(ANISO)
    e = E.Engine(0)
    try:
        e.upload(m); e.set_reparametrization(ANISO)
        for n in (2, 3, 1):
            _new_form(_timed_pass(e, o, n), n, n)
            assert np.array_equal(e.download_duals(), o.duals()), n
        lb, lbo = e.lower_bound(), o.LowerBound()
        assert abs(lb - lbo) <= LB_RTOL * abs(lbo)
    finally:
        e.close()
