"""Labeling messages whose left factor has SEVERAL labelings, on every kernel path that runs them (the models: tests/labeling_cases.py;
why they can tell, and the census of kernel bodies: tests/test_labeling_shapes_host.py).  Every labeling-list model of the other
test files has one left labeling and one index per table, so ``nl = Op::pd1 = 1`` in all they run: ``dl(0)`` for ``dl(tab[r])``, an
``l`` loop run once, ``D[q][k][j]`` for ``D[q][k][l]``, a wrong ``len`` or a table read as the identity pass there.

The yardstick is the one of tests/test_op_caps_gpu.py: the oracle on identical input, duals ``np.array_equal`` after every call, the
bound within 1e-9 relative, the factors' bounds within 1e-12; the class split is asserted before anything runs.  Four engines must
agree with the oracle: the defaults (level loop), LPMP_NO_LEVEL_LOOP=1 (graph replay of sweep_generic_kernel<1> / <64>),
LPMP_CHAIN_ALL=1 (chain_generic_kernel tickets) and LPMP_NO_CHAIN=1 (plain launches)."""
import numpy as np
import pytest

from lp_mp_amd import model as M
from lp_mp_amd import engine as E
from oracle.binding import Oracle

import labeling_cases as LC
from test_fuzz_gpu import random_rows

pytestmark = pytest.mark.gpu

LB_RTOL = 1e-9
FLB_ATOL = 1e-12
CALLS = LC.CALLS
# name -> environment: LPMP_NO_CHAIN is read when an engine is created, the others whenever a schedule is planned
ENGINES = LC.ENGINES


@pytest.fixture(scope="module")
def engines():
    """one engine per way of running a sweep; "plain launches" is created under its variable"""
    import os
    out = {}
    for name, env in ENGINES:
        nc = env.get("LPMP_NO_CHAIN")
        if nc:
            os.environ["LPMP_NO_CHAIN"] = nc
        try:
            out[name] = E.Engine(0)
        finally:
            os.environ.pop("LPMP_NO_CHAIN", None)
    yield out
    for e in out.values():
        e.close()


_call = LC.call


_MODELS, _REFERENCE = {}, {}


def _model(name, flags=0):
    if (name, flags) not in _MODELS:
        _MODELS[(name, flags)] = LC.case(name, flags)
    return _MODELS[(name, flags)]


def _reference(name, mode, rtype, flags=0):
    """the oracle over CALLS, computed once per (case, mode, send rule) and left unchanged: duals and bound after every call, the
    factors' bounds at the end"""
    key = (name, mode, rtype, flags)
    if key not in _REFERENCE:
        m = _model(name, flags)
        o = Oracle(m)
        o.set_reparametrization_type(rtype); o.set_reparametrization(mode)
        steps = []
        for what, n in CALLS:
            _call(o, what, n)
            d = o.duals().copy(); d.setflags(write=False)
            assert np.all(np.isfinite(d)), (name, mode, rtype, what, n)
            steps.append((d, o.LowerBound()))
        flb = np.array([o.factor_lower_bound(f) for f in range(m.n_factors)]); flb.setflags(write=False)
        _REFERENCE[key] = (steps, flb)
    return _REFERENCE[key]


def _same(e, duals, bound, what):
    d = e.download_duals()
    assert np.array_equal(d, duals), (what, float(np.max(np.abs(d - duals))), int(np.sum(d != duals)))
    lb = e.lower_bound()
    assert abs(lb - bound) <= LB_RTOL * max(1.0, abs(bound)), (what, lb, bound)


def _set_env(monkeypatch, c, env):
    for k in ("LPMP_NO_LEVEL_LOOP", "LPMP_CHAIN_ALL", "LPMP_CHAIN_MIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if k != "LPMP_NO_CHAIN":
            monkeypatch.setenv(k, v)
    if c.chain_min:
        monkeypatch.setenv("LPMP_CHAIN_MIN", str(c.chain_min))


def _run(engines, monkeypatch, name, rtype, modes=LC.MODES, flags=0):
    c = LC.CASES[name]
    m = _model(name, flags)
    for which, env in ENGINES:
        e = engines[which]
        _set_env(monkeypatch, c, env)
        e.set_reparametrization_type(rtype)
        try:
            for mode in modes:
                steps, flb = _reference(name, mode, rtype, flags)
                e.upload(m)
                e.set_reparametrization(mode)
                if mode == modes[0] and rtype in (M.RTYPE_SHARED, M.RTYPE_RESIDUAL):
                    LC.assert_path(e.plan, c, which)
                for k, ((what, n), (duals, bound)) in enumerate(zip(CALLS, steps)):
                    _call(e, what, n)
                    _same(e, duals, bound, (name, which, mode, rtype, k, what, n))
                assert np.max(np.abs(e.factor_lower_bounds() - flb)) <= FLB_ATOL, (name, which, mode, rtype)
        finally:
            e.set_reparametrization_type(0)


@pytest.mark.parametrize("name", list(LC.CASES))
def test_shared_send_rule_equals_the_oracle_on_four_engines(engines, monkeypatch, name):
    _run(engines, monkeypatch, name, M.RTYPE_SHARED)


@pytest.mark.parametrize("name", list(LC.CASES))
def test_residual_send_rule_equals_the_oracle_on_four_engines(engines, monkeypatch, name):
    """the residual rule keeps every launch of the level loop off the lane-per-op bodies (generic_body<1> between the barriers)"""
    _run(engines, monkeypatch, name, M.RTYPE_RESIDUAL)


ADAPTIVE = [n for n, c in LC.CASES.items() if c.family in ("pair_trip7", "perm8", "gen9x20") and c.shape == "chain" and c.io == c.fam.io]


@pytest.mark.parametrize("name", ADAPTIVE)
def test_adaptive_send_rule_equals_the_oracle_on_four_engines(engines, monkeypatch, name):
    """MF_IMPROVEMENT on the message types: the OP_LABELING branch of ``improvement`` (kernels.hip), with the updated factor on the
    left (schedules left, full, only send) and on the right (right, full, only send)"""
    assert {LC.CASES[n].sched for n in ADAPTIVE if LC.CASES[n].family == LC.CASES[name].family} >= {"left", "full"}
    _run(engines, monkeypatch, name, M.RTYPE_ADAPTIVE, flags=M.MF_IMPROVEMENT)


RANGE_CASES = [c.name for c in LC.SMALL_CASES if c.shape in ("chain", "random", "dup", "hub8", "copies9", "copies16", "copies17")]


@pytest.mark.parametrize("name", RANGE_CASES)
def test_random_iterator_range_passes(engines, monkeypatch, name):
    """random factor subsets, receive masks and weights (``random_rows`` of tests/test_fuzz_gpu.py): records with n_recv != n_send,
    and sends whose peer a receive of the same record has just rewritten — in label_ops_body_staged the receive's lane hands the
    rewritten costs over in LDS (Op::pad) — beside sends to peers no receive touched"""
    c = LC.CASES[name]
    m = _model(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    o = Oracle(m)
    rows = [random_rows(rng, None, o, m) for _ in range(4)]
    want = []
    for r in rows:
        o.compute_pass_custom(*r)
        d = o.duals().copy()
        assert np.all(np.isfinite(d)), name
        want.append((d, o.LowerBound()))
    for which, env in ENGINES:
        e = engines[which]
        _set_env(monkeypatch, c, env)
        monkeypatch.setenv("LPMP_CHAIN_MIN", "2")
        e.upload(m)
        e.set_reparametrization(M.REPAM_ANISOTROPIC)
        for k, (r, (d, lb)) in enumerate(zip(rows, want)):
            e.compute_pass_custom(*r)
            _same(e, d, lb, (name, which, k))


def test_lower_bound_of_mixed_implicit_origins_and_long_vectors(engines):
    """``lower_bound()`` and the factors' bounds before and after a pass, on vector factors of 1, 64, 65 and 512 entries with and
    without an implicit origin (factor_lb in factor_lb_kernel / factor_lb_list_kernel): costs of both signs, so that the origin
    decides some bounds and not others"""
    fams = [LC.synthetic_family("lb%d" % n, nl, n, 1, 1, "generic", seed=50 + n) for nl, n in ((1, 64), (64, 65), (65, 512))]
    mt = [M.MsgType(2 * k, 2 * k + 1, M.SCHED_LEFT, 0, 0, M.M_LABELING, k) for k in range(3)]
    b = M.ModelBuilder(6, mt)
    for f in fams:
        b.add_labeling_table(f.left, f.right, f.indices[0])
    rng = np.random.default_rng(7)
    for k, f in enumerate(fams):
        for lio, rio in ((False, True), (True, False), (True, True), (False, False)):
            lo = 0.2 if rng.integers(2) else -1.0           # all costs above 0: only the origin gives the bound 0
            l = b.add_vector_factors(2 * k, rng.uniform(lo, 1, (2, f.nl)), implicit_origin=lio)
            r = b.add_vector_factors(2 * k + 1, rng.uniform(lo, 1, (2, f.nr)), implicit_origin=rio)
            for a in range(2):
                for x in range(2):
                    b.add_messages(k, l[a], r[x]); b.add_relations(l[a], r[x])
    m = b.finish()
    assert sorted(set(m.f_dim0.tolist())) == [1, 64, 65, 512] and set(m.f_flags.tolist()) == {0, 1}
    for e in (engines["level loop"], engines["plain launches"]):
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            o = Oracle(m); o.set_reparametrization(mode)
            e.upload(m); e.set_reparametrization(mode)
            for step in range(3):
                if step:
                    o.ComputePass(1); e.compute_pass(1)
                    assert np.array_equal(e.download_duals(), o.duals()), (mode, step)
                lb, want = e.lower_bound(), o.LowerBound()
                assert abs(lb - want) <= LB_RTOL * max(1.0, abs(want)), (mode, step, lb, want)
                flb = np.array([o.factor_lower_bound(f) for f in range(m.n_factors)])
                assert np.max(np.abs(e.factor_lower_bounds() - flb)) <= FLB_ATOL, (mode, step)


@pytest.mark.parametrize("name", [c.name for c in LC.SMALL_CASES if c.shape == "dup"])
def test_receive_and_send_on_one_peer_through_two_tables(engines, monkeypatch, name):
    """an iterator-range pass over the left factors in which the factor joined to ONE right factor through TWO tables receives
    through the first and sends through the second: the send needs the costs that receive has just rewritten.  (The staged body
    of the level loop requested them together with the receive's and sent stale costs back — found by
    test_random_iterator_range_passes[many_to_one dup left io00]; such a launch now stays on the op-by-op body.)"""
    c = LC.CASES[name]
    m = _model(name)
    o = Oracle(m)
    off, ent = o.msg_lists()
    n_left = int(np.sum(m.f_type == 0))
    om, mk, oo, mo, hit = [], [], [0], [0], 0
    for f in range(n_left):
        msgs = [int(x) // 2 for x in ent[off[f]: off[f + 1]]]
        peers = [int(m.m_right[g]) for g in msgs]
        for k, p in enumerate(peers):
            twice = peers.count(p) == 2
            first = twice and peers.index(p) == k
            hit += twice
            mk.append(0 if twice and not first else 1)
            om.append(0.0 if first else 0.5 / len(peers))
        oo.append(len(om)); mo.append(len(mk))
    assert hit == 2
    rows = (np.arange(n_left, dtype=np.int32), np.array(oo, np.int64), np.array(om), np.array(mo, np.int64), np.array(mk, np.uint8))
    want = []
    for k in range(2):
        o.compute_pass_custom(*rows)
        want.append((o.duals().copy(), o.LowerBound()))
    assert np.all(np.isfinite(want[-1][0]))
    for which, env in ENGINES:
        e = engines[which]
        _set_env(monkeypatch, c, env)
        monkeypatch.setenv("LPMP_CHAIN_MIN", "2")
        e.upload(m)
        e.set_reparametrization(M.REPAM_ANISOTROPIC)
        if which == "level loop":
            info = e.plan.custom_schedule_info(*rows)
            assert info["n_levels"] >= 2, info
        for k, (d, lb) in enumerate(want):
            e.compute_pass_custom(*rows)
            _same(e, d, lb, (name, which, k))
