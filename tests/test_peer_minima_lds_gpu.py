"""Peer minima with a publishing record's first table parked in LDS (kernels.hip dense_pq_publish_body<L, 2, S>): a W record
with more than two receives writes table 0 to its wave's LDS area before the second pair of tables takes the registers, and reads it
back for the publish; only table 1 is requested again, and not even that with three receives.  ``LPMP_PQ_LDS=0`` selects the form that
requests both again.  Every case, in both forms: duals ``np.array_equal`` to the CPU oracle, the bound within 1e-9 relative, and
``peer_minima_launches`` equal to the chain launches.  Tables are random per edge, so a mixed-up slot shows."""
import numpy as np
import pytest

from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from lp_mp_amd import engine as E
from oracle.binding import Oracle

pytestmark = pytest.mark.gpu

ANISO = M.REPAM_ANISOTROPIC
LB_RTOL = 1e-9
NAME = "chain_dense_pk_kernel<32, 2, false, false>"          # the class's name in the timing, whichever form ran
PASSES = (1, 2, 5, 9, 33)                                     # explicit lists, the periodic template, a slice of 32 + 1
FORMS = [None, "0"]                                           # LPMP_PQ_LDS unset (parked) / 0 (both requested again)


def _setup(monkeypatch, form, window, tiles=None):
    bands, lag, depth = window
    monkeypatch.setenv("LPMP_ROT_BANDS", str(bands)); monkeypatch.setenv("LPMP_ROT_LAG", str(lag)); monkeypatch.setenv("LPMP_ROT_DEPTH", str(depth))
    if tiles is not None:
        monkeypatch.setenv("LPMP_ROT_TILES", str(tiles))
    if form is None:
        monkeypatch.delenv("LPMP_PQ_LDS", raising=False)
    else:
        monkeypatch.setenv("LPMP_PQ_LDS", form)


def _timed_pass(e, o, n):
    e.enable_kernel_timing(True); e.reset_kernel_timing()
    e.compute_pass(n)
    if o is not None:
        o.ComputePass(n)
    kt = e.kernel_timing(); e.reset_kernel_timing(); e.enable_kernel_timing(False)
    return kt


def _new_form(kt, n, what=None):
    (v,) = kt.values()
    assert v["kernel"] == NAME, (what, kt)
    assert v["chain_launches"] == (n + 31) // 32 and v["peer_minima_launches"] == v["chain_launches"], (what, kt)


def _same(e, o, what=None):
    d, do = e.download_duals(), o.duals()
    assert np.array_equal(d, do), (what, float(np.max(np.abs(d - do))))
    lb, lbo = e.lower_bound(), o.LowerBound()
    assert abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (what, lb, lbo)


def _run(m, passes, what):
    o = Oracle(m); o.set_reparametrization(ANISO)
    e = E.Engine(0)
    try:
        e.upload(m); e.set_reparametrization(ANISO)
        assert e.plan.pass_rotates(ANISO)
        for n in passes:
            _new_form(_timed_pass(e, o, n), n, (what, n))
            _same(e, o, (what, n))
    finally:
        e.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bands,lag,depth", [(8, 2, 4), (5, 1, 2)])
@pytest.mark.parametrize("H,W", [(4, 5), (5, 5), (13, 11), (40, 36)])
def test_records_with_two_three_and_four_receives(H, W, bands, lag, depth, form, monkeypatch):
    """either colour holds W records with 2, 3 and 4 receives; 5 x 5 leaves a last workgroup with dead record slots; over the pass
    counts a wave's LDS area is reused across tickets and roles, a 4-receive record followed by a 3-receive one in the same slot"""
    _setup(monkeypatch, form, (bands, lag, depth))
    _run(S.grid_model(H, W, 32, order="colour_major", seed=1000 + H * W + bands), PASSES, (H, W, form))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("H,W", [(1, 7), (2, 2)])
def test_records_with_at_most_two_receives(H, W, form, monkeypatch):
    """nothing is parked: the second pair of tables does not exist"""
    _setup(monkeypatch, form, (8, 2, 4))
    _run(S.grid_model(H, W, 32, order="colour_major", seed=2000 + H * W), PASSES, (H, W, form))


def _hard(m, L, seed, frac=0.35):
    """+inf entries in the tables; the diagonal stays finite, so every row and column keeps a finite entry (tests/test_peer_minima_gpu.py)"""
    rng = np.random.default_rng(seed)
    T = np.asarray(m.const_data).reshape(-1, L, L)
    mask = rng.random(T.shape) < frac
    mask[:, np.arange(L), np.arange(L)] = False
    T[mask] = np.inf
    return m


@pytest.mark.parametrize("form", FORMS)
def test_hard_constraints(form, monkeypatch):
    _setup(monkeypatch, form, (5, 1, 2))
    m = _hard(S.grid_model(13, 11, 32, order="colour_major", seed=67), 32, 67)
    o = Oracle(m); o.set_reparametrization(ANISO)
    e = E.Engine(0)
    try:
        e.upload(m); e.set_reparametrization(ANISO)
        for n in (1, 3, 9):
            _new_form(_timed_pass(e, o, n), n, (form, n))
            assert np.isfinite(e.download_duals()).all()
            _same(e, o, (form, n))
    finally:
        e.close()


@pytest.mark.parametrize("form", FORMS)
def test_tiled_order(form, monkeypatch):
    _setup(monkeypatch, form, (8, 2, 4), tiles=3)
    _run(S.grid_model(13, 11, 32, order="colour_major", seed=79), PASSES, ("tiled", form))


def test_both_forms_equal_bit_for_bit(monkeypatch):
    """14 x 10, 9 passes: duals and factor_lower_bounds() of the parked form and of the form that requests both tables again"""
    m = S.grid_model(14, 10, 32, order="colour_major", seed=14)
    got = []
    for form in FORMS:
        _setup(monkeypatch, form, (8, 2, 4))
        e = E.Engine(0)                                       # (the switch is read when the engine is created)
        try:
            e.upload(m); e.set_reparametrization(ANISO)
            _new_form(_timed_pass(e, None, 9), 9, form)
            got.append((e.download_duals(), e.factor_lower_bounds()))
        finally:
            e.close()
    assert np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1], got[1][1])
