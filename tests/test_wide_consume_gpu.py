"""Peer-minima launches in the wide consume form (kernels.hip dense_pq_consume_body on 32-lane groups): a wave carries two
H / K / T records, a consume ticket eight, planned from block relations of their own (order.cpp plan_rotation_chain, consume_gpb).
Every case runs the same calls on the CPU oracle, on an engine in the wide form (the default) and on one with ``LPMP_PQ_WIDE=0`` (four
records per consume ticket, as before): duals ``np.array_equal`` among all three, the bound within 1e-9 relative, every chain launch a
peer-minima launch, and the engine's own report (LPMP_ROT_VERBOSE) names the form that ran.

Consume records (colour 0) of the grids: 1 x 7: 4 (H, K, T: less than one block); 3 x 3: 5 (a block with dead lane groups, and a wave
with a live and a dead record); 13 x 11: 72; 14 x 10: 70 (a last block of six); 40 x 36: 720 — corner, border and inner records (2, 3 and
4 receives) share waves in all of them."""
import dataclasses
import re

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
GRIDS = [(1, 7), (3, 3), (13, 11), (14, 10), (40, 36)]
PASSES = (1, 2, 3, 5, 9, 12)                 # 9 and 12: the periodic template of either parity (where the depth is even)
FORM = re.compile(r"LPMP_PQ_WIDE=(\d): (\d+) records per consume ticket")


def _window(monkeypatch, bands, lag, depth):
    monkeypatch.setenv("LPMP_ROT_BANDS", str(bands)); monkeypatch.setenv("LPMP_ROT_LAG", str(lag)); monkeypatch.setenv("LPMP_ROT_DEPTH", str(depth))


class Trio:
    """the oracle, the wide engine and the LPMP_PQ_WIDE=0 engine on one model (the switch is read when an engine is created)"""

    def __init__(self, m, monkeypatch, mode=ANISO, **upload):
        monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
        self.o = Oracle(m); self.o.set_reparametrization(mode)
        self.wide = self.old = None
        monkeypatch.delenv("LPMP_PQ_WIDE", raising=False)
        self.wide = E.Engine(0)
        monkeypatch.setenv("LPMP_PQ_WIDE", "0")
        self.old = E.Engine(0)
        monkeypatch.delenv("LPMP_PQ_WIDE")
        for e in (self.wide, self.old):
            e.upload(m, **upload); e.set_reparametrization(mode)

    def engines(self):
        return (("wide", self.wide), ("old", self.old))

    def compute_pass(self, n):
        """n passes on all three; every chain launch of either engine must have been a peer-minima launch"""
        self.o.ComputePass(n)
        for name, e in self.engines():
            e.enable_kernel_timing(True); e.reset_kernel_timing()
            e.compute_pass(n)
            kt = e.kernel_timing(); e.reset_kernel_timing(); e.enable_kernel_timing(False)
            (v,) = kt.values()
            assert v["chain_launches"] == (n + 31) // 32 and v["peer_minima_launches"] == v["chain_launches"], (name, n, kt)

    def same(self, what=None):
        do, lbo = self.o.duals(), self.o.LowerBound()
        dw = self.wide.download_duals()
        assert np.array_equal(dw, do), ("wide against the oracle", what, float(np.max(np.abs(dw - do))))
        assert np.array_equal(dw, self.old.download_duals()), ("wide against LPMP_PQ_WIDE=0", what)
        for name, e in self.engines():
            lb = e.lower_bound()
            assert abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (name, what, lb, lbo)

    def close(self):
        for e in (self.wide, self.old):
            if e is not None:
                e.close()


def _forms(capfd):
    """the (LPMP_PQ_WIDE, records per consume ticket) pairs the engines reported since the last call"""
    return set(FORM.findall(capfd.readouterr().err))


@pytest.mark.parametrize("H,W", GRIDS)
@pytest.mark.parametrize("bands,lag,depth", WINDOWS)
def test_bit_parity_on_small_grids(H, W, bands, lag, depth, monkeypatch, capfd):
    _window(monkeypatch, bands, lag, depth)
    m = S.grid_model(H, W, 32, order="colour_major", seed=3 * H * W + bands)
    t = Trio(m, monkeypatch)
    try:
        capfd.readouterr()
        for n in PASSES:
            t.compute_pass(n)
            t.same((H, W, n))
        assert _forms(capfd) == {("1", "8"), ("0", "4")}
        flb = t.wide.factor_lower_bounds()
        assert np.max(np.abs(flb - np.array([t.o.factor_lower_bound(f) for f in range(m.n_factors)]))) <= 1e-12
    finally:
        t.close()


@pytest.mark.parametrize("H,W", [(13, 11), (40, 36)])
def test_tiled_order(H, W, monkeypatch, capfd):
    _window(monkeypatch, 8, 2, 4)
    monkeypatch.setenv("LPMP_ROT_TILES", "3")
    t = Trio(S.grid_model(H, W, 32, order="colour_major", seed=78), monkeypatch)
    try:
        capfd.readouterr()
        for n in PASSES:
            t.compute_pass(n)
            t.same(n)
        err = capfd.readouterr().err
        assert "tiled order" in err and set(FORM.findall(err)) == {("1", "8"), ("0", "4")}
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
    t = Trio(_hard(S.grid_model(13, 11, 32, order="colour_major", seed=62), 32, 62), monkeypatch)
    try:
        for n in (1, 3, 9):
            t.compute_pass(n)
            assert np.isfinite(t.wide.download_duals()).all()
            t.same(n)
        assert ("1", "8") in _forms(capfd)
    finally:
        t.close()


def test_per_pass_bound_rows(monkeypatch, capfd):
    """speculative batches: one pass and its bound per call, the passes run ahead as one joined launch with a bound row per seam — the
    HIST_MID stores of the consume body sit behind reductions that both records of a wave must reach"""
    _window(monkeypatch, 8, 2, 4)
    t = Trio(S.grid_model(14, 10, 32, order="colour_major", seed=10), monkeypatch)
    try:
        for _, e in t.engines():
            e.set_speculation(8); e.reset_kernel_timing()          # (timing stays off: a timed engine does not run ahead)
        for k in range(21):
            t.o.ComputePass(1)
            lbo = t.o.LowerBound()
            for name, e in t.engines():
                e.compute_pass(1)
                lb = e.lower_bound()
                assert abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (name, k, lb, lbo)
        for name, e in t.engines():
            st = e.speculation_stats()
            assert st["batches"] > 0 and st["passes_launched"] >= 21, (name, st)
            assert e.peer_minima_launches() >= st["batches"], name
            e.set_speculation(0)
        t.same()
        assert _forms(capfd) == {("1", "8"), ("0", "4")}
    finally:
        t.close()


def test_nothing_published_is_read_across_calls(monkeypatch, capfd):
    """two calls with new tables in between: the minima published by the first are never read by the second"""
    _window(monkeypatch, 8, 2, 4)
    m = S.grid_model(13, 11, 32, order="colour_major", seed=4)
    t = Trio(m, monkeypatch)
    try:
        t.compute_pass(3)
        t.same("before")
        const = 0.25 + S.u01(np.asarray(m.const_data).shape[0], 994)
        for _, e in t.engines():
            e.upload_costs(const=const)
        d = t.o.duals()
        t.o = Oracle(dataclasses.replace(m, const_data=const, _keep=[])); t.o.set_reparametrization(ANISO); t.o.set_duals(d)
        t.compute_pass(5)
        t.same("after upload_costs")
        assert ("1", "8") in _forms(capfd)
    finally:
        t.close()


def test_medium_size_without_override(monkeypatch, capfd):
    """384 x 384 (2.4 GB of tables, above the engine's 1 GiB threshold): the engine's own choice is the wide form"""
    t = Trio(S.grid_model(384, 384, 32, order="colour_major", seed=6), monkeypatch)
    try:
        for n in (3, 1):
            t.compute_pass(n)
            t.same(n)
        assert _forms(capfd) == {("1", "8"), ("0", "4")}
    finally:
        t.close()


@pytest.mark.parametrize("L,f32,name", [(16, False, "chain_dense_pk_kernel<16, 2, false, false>"),
                                       (32, True, "chain_dense_pk_f32_kernel<32, 2, false, false>")])
def test_other_classes_keep_their_kernels(L, f32, name, monkeypatch, capfd):
    """16 labels, and 32 labels on float tables: no peer minima, the old kernels on the plan's own block relations"""
    _window(monkeypatch, 8, 2, 4)
    monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
    m = S.grid_model(14, 10, L, order="colour_major", seed=L + 1)
    if f32:
        c = np.asarray(m.const_data); c[:] = c.astype(np.float32)               # float-valued costs: exact in float storage
    o = Oracle(m); o.set_reparametrization(ANISO)
    e = E.Engine(0)
    try:
        e.upload(m, table_precision="f32" if f32 else None); e.set_reparametrization(ANISO)
        for n in (2, 5):
            e.enable_kernel_timing(True); e.reset_kernel_timing()
            e.compute_pass(n); o.ComputePass(n)
            kt = e.kernel_timing(); e.reset_kernel_timing(); e.enable_kernel_timing(False)
            assert [v["kernel"] for v in kt.values()] == [name], kt
            assert all(v["chain_launches"] == 1 and v.get("peer_minima_launches", 0) == 0 for v in kt.values()), kt
            assert np.array_equal(e.download_duals(), o.duals()), n
        assert e.peer_minima_launches() == 0 and not _forms(capfd)
    finally:
        e.close()
