"""The banded form of class ``diff`` without a GPU: band detection (the planner against ``model.diff_band``), the rule, which
launches take the banded kernel, the exactness of the banded reduction (numpy, bit for bit), and the oracle over every expansion
tests/test_diff_band_gpu.py compares the device with."""
import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import diff_band_cases as C


def _chain(vectors):
    """a chain with one L x L DIFF factor per vector (n = 2L - 1 entries each; a 1-entry vector: a 1 x 1 factor)"""
    dims = [(len(D) + 1) // 2 for D in vectors]
    mt, ft = [], {}
    for L in sorted(set(dims)):
        ft[L] = (len(ft) * 2, len(ft) * 2 + 1)
    for L, (fu, fp) in ft.items():
        mt += [M.MsgType(fu, fp, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(fu, fp, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1)]
    mt_of = {L: 2 * i for i, L in enumerate(ft)}
    b = M.ModelBuilder(2 * len(ft), mt)
    rng = np.random.default_rng(5)
    for D, L in zip(vectors, dims):
        t = b.add_diff_table(D)
        u = [int(b.add_vector_factors(ft[L][0], rng.uniform(0, 1, (1, L)))[0]) for _ in range(2)]
        p = int(b.add_diff_pairwise(ft[L][1], L, L, [t], [1.25])[0])
        b.add_messages(mt_of[L], u[0], p)
        b.add_messages(mt_of[L] + 1, u[1], p)
        b.add_relations([u[0], p], [p, u[1]])
    return b.finish()


def _detection_vectors():
    L = 20
    n = 2 * L - 1
    v = []
    for trunc in (1, 2, 5, 19, 100):
        v.append(M.truncated_linear(L, L, 0.3, 0.3 * trunc))
        v.append(M.truncated_quadratic(L, L, 0.02, 0.02 * trunc * trunc))
    v.append(C.band_vector(L, L, -2, 1, 1.5, 2.25))                    # unequal tails
    v.append(C.band_vector(L, L, -1, 1, np.inf, np.inf))                # +inf tails
    v.append(C.band_vector(L, L, -3, 3, np.inf, 2.0))
    v.append(C.band_vector(L, L, L - 5, L - 1, 1.75, 0.0))              # a left tail only
    v.append(C.band_vector(L, L, -(L - 1), -(L - 1) + 3, 0.0, 0.0))     # a right tail only
    v.append(np.full(n, 0.75))                                          # constant
    v.append(np.full(n, np.inf))
    v.append(S.u01(n, 3))                                               # no tail
    z = np.zeros(n); z[L - 1] = 1.0; z[3] = -0.0; v.append(z)           # a left tail of +0.0 interrupted by -0.0
    z = np.zeros(n); z[L - 1] = 1.0; z[n - 4] = -0.0; v.append(z)       # the right tail
    z = np.full(n, -0.0); z[0] = 0.0; v.append(z)                       # +0.0 first, -0.0 from there on
    v.append(np.array([2.0, 2.0, 3.0, 3.0, 3.0]))                       # two tails that meet: an empty band between them
    v.append(np.array([0.5]))                                           # 1 entry
    return v


def test_detection_equals_the_numpy_statement():
    vs = _detection_vectors()
    assert M.diff_band(vs[-1]) == (1, 0) and M.diff_band(vs[-2]) == (2, 1) and M.diff_band(np.full(7, 1.0)) == (7, 6)
    z = np.zeros(9); z[2] = -0.0; z[4] = 1.0
    assert M.diff_band(z) == (2, 4)                                     # by bits: -0.0 is not +0.0
    p = E.Plan(_chain(vs))
    bands = p.diff_bands()
    assert sorted(bands) == list(range(len(vs)))
    for t, D in enumerate(vs):
        lo, hi = M.diff_band(D)
        assert bands[t] == (lo, hi, M.diff_band_is_banded(D)), (t, bands[t], lo, hi)
        assert np.all(D[:lo].view(np.uint64) == D[:1].view(np.uint64)) and np.all(D[hi + 1:].view(np.uint64) == D[-1:].view(np.uint64))
        assert hi - lo + 1 >= 0
    # every model of the GPU tests
    for name, m in [("mid", C.mid_grid())] + [x for i, x in enumerate(C.gpu_expansion_cases()) if i % 7 == 0]:
        if not m.has_diff:
            continue
        bands = E.Plan(m).diff_bands()
        ts = sorted({int(t) for t in m.f_table[m.f_kind == M.F_PAIRWISE_DIFF]})
        assert sorted(bands) == ts, name
        for t in ts:
            D = m.shared_table(t).reshape(-1)
            assert bands[t] == M.diff_band(D) + (M.diff_band_is_banded(D),), (name, t)


def test_tables_no_diff_factor_references_have_no_band():
    m = S.grid_model(5, 4, 8, pairwise="shared")
    assert E.Plan(m).diff_bands() == {}
    assert E.Plan(S.grid_model(5, 4, 8, pairwise="dense")).diff_bands() == {}


@pytest.mark.parametrize("L", (8, 33, 64, 130))
def test_the_rule(L):
    """a width of exactly n / DIFF_BAND_DIV (rounded down) is banded, one entry more is not"""
    n = 2 * L - 1
    w = C.widest(L)
    assert w * M.DIFF_BAND_DIV <= n < (w + 1) * M.DIFF_BAND_DIV
    for extra, want in ((0, True), (1, False)):
        m = C.band_grid(L, "colour_major", (C.centred(w + extra),) * 2, shape=(4, 3))
        p = E.Plan(m)
        for t, (lo, hi, banded) in p.diff_bands().items():
            assert hi - lo + 1 == w + extra and banded == want, (L, t, lo, hi, banded)
        for d in (0, 1):
            info = p.diff_band_info(d, M.REPAM_ANISOTROPIC)
            assert info["diff_launches"] > 0 and info["band_launches"] == (info["diff_launches"] if want else 0), info
            assert info["band_receives"] == (info["diff_receives"] if want else 0) and info["diff_receives"] > 0


@pytest.mark.parametrize("order", C.ORDERS)
def test_which_launches_are_banded(order, monkeypatch):
    trunc = C.truncated_grid("linear", 40, 2, order)                    # all vectors truncated
    mixed = C.mixed_level_grid(order)                                   # one truncated, one random, in every level
    assert C.banded(trunc) and not C.banded(mixed)
    n_upd = 42
    plans = [(E.Plan(trunc), True), (E.Plan(mixed), False)]
    monkeypatch.setenv("LPMP_NO_DIFF_BAND", "1")
    plans.append((E.Plan(trunc), False))                                # the switch is read as the plan is made
    monkeypatch.delenv("LPMP_NO_DIFF_BAND")
    for m, (p, want) in zip((trunc, mixed, trunc), plans):
        x = E.Plan(m.expand_diff())
        for d in (0, 1):
            for mode in C.MODES:
                info = p.diff_band_info(d, mode)
                assert info["diff_launches"] > 0 and info["band_launches"] == (info["diff_launches"] if want else 0), (d, mode, info)
                assert info["band_receives"] == (info["diff_receives"] if want else 0)
                assert p.schedule_classes(d, mode) == {"diff": n_upd}
                ip, ix = p.schedule_info(d, mode), x.schedule_info(d, mode)
                assert info["diff_launches"] == ip["n_launches"] and info["diff_receives"] == ip["n_receives"]
                for k in ("n_levels", "n_launches", "n_receives", "n_sends"):
                    assert ip[k] == ix[k], (k, ip, ix)
    # the detection itself does not depend on the switch
    assert plans[0][0].diff_bands() == plans[2][0].diff_bands()
    # levels, records and bytes are those of the plan without the banded kernel
    for d in (0, 1):
        for mode in C.MODES:
            assert plans[0][0].schedule_info(d, mode) == plans[2][0].schedule_info(d, mode)
            assert np.array_equal(plans[0][0].update_levels(d, mode), plans[2][0].update_levels(d, mode))


def test_a_launch_with_one_unbanded_receive_is_not_banded():
    """two levels of a chain: u0 - p0 - u1 - p1 - u2 with p0 banded and p1 random: u1 receives from both"""
    L = 12
    p = E.Plan(_chain_of([C.band_vector(L, L, -1, 1), S.u01(2 * L - 1, 9)], L))
    info = [p.diff_band_info(d, M.REPAM_UNIFORM) for d in (0, 1)]
    assert all(i["diff_launches"] > 0 for i in info)
    assert all(i["band_launches"] < i["diff_launches"] for i in info), info
    q = E.Plan(_chain_of([C.band_vector(L, L, -1, 1), C.band_vector(L, L, 0, 2, seed=4)], L))
    for d in (0, 1):
        i = q.diff_band_info(d, M.REPAM_UNIFORM)
        assert i["band_launches"] == i["diff_launches"] > 0


def _chain_of(vectors, L):
    mt = [M.MsgType(0, 1, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(0, 1, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1)]
    b = M.ModelBuilder(2, mt)
    rng = np.random.default_rng(2)
    u = [int(b.add_vector_factors(0, rng.uniform(0, 1, (1, L)))[0]) for _ in range(len(vectors) + 1)]
    for i, D in enumerate(vectors):
        p = int(b.add_diff_pairwise(1, L, L, [b.add_diff_table(D)], [0.75])[0])
        b.add_messages(0, u[i], p)
        b.add_messages(1, u[i + 1], p)
        b.add_relations([u[i], p], [p, u[i + 1]])
    return b.finish()


N_SHARDS = 6


@pytest.mark.parametrize("shard", range(N_SHARDS))
def test_the_banded_reduction_is_the_full_one_bit_for_bit(shard):
    """for every (vector, dims, scale) of the GPU models and four kinds of m_o, both sides: the window and the two tail terms give
    the bytes of the minimum over all pairs.  (The minimum is the device's: -0.0 below +0.0.)"""
    cases = C.receive_cases()
    assert sum(len(c[3]) for c in cases) > 800
    for D, d0, d1, scales in cases[shard::N_SHARDS]:
        for side in (0, 1):
            oth = d1 if side == 0 else d0
            for mo in C.other_side_vectors(oth, d0 * 1000 + d1):
                for sc in scales:
                    a = C.minplus_full(D, d0, d1, sc, mo, side)
                    b = C.minplus_banded(D, d0, d1, sc, mo, side)
                    assert a.tobytes() == b.tobytes(), (d0, d1, side, sc, M.diff_band(D))


def test_the_banded_reduction_on_random_vectors():
    """the statement itself on what the models do not hold: any band, tails of 0.0 / -0.0 / +inf, integer entries, rectangular dims"""
    rng = np.random.default_rng(11)
    for _ in range(300):
        d0, d1 = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        n = d0 + d1 - 1
        w = int(rng.integers(0, n + 1)); lo = int(rng.integers(0, n - w + 1))
        D = np.empty(n)
        D[:lo] = rng.choice([0.0, -0.0, 1.5, np.inf]); D[lo + w:] = rng.choice([0.0, 2.0, -1.0, np.inf]); D[lo:lo + w] = rng.integers(-2, 3, w)
        sc = float(rng.choice([1.0, -0.75, 0.0, 1.3]))
        if np.isinf(D).any() and sc <= 0:
            sc = 1.0
        for side in (0, 1):
            for mo in C.other_side_vectors(d1 if side == 0 else d0, int(rng.integers(1 << 30))):
                assert C.minplus_full(D, d0, d1, sc, mo, side).tobytes() == C.minplus_banded(D, d0, d1, sc, mo, side).tobytes(), (d0, d1, side, sc, D)


def test_expectations_of_the_gpu_cases():
    """what the GPU tests assert before anything runs, from the numpy statement of the rule: which models are banded"""
    for L in C.GRID_LABELS:
        for r in C.HALF_WIDTHS:
            assert C.banded(C.label_grid(L, "row_major", r)) == ((2 * r + 1) * M.DIFF_BAND_DIV <= 2 * L - 1)
            assert (L, r) == (8, 2) or C.banded(C.label_grid(L, "row_major", r))
    for L in C.RULE_LABELS:
        assert C.banded(C.rule_grid(L, "row_major", 0)) and not C.banded(C.rule_grid(L, "row_major", 1))
    for kind in C.ASYM_KINDS:
        for L in C.ASYM_LABELS:
            assert C.banded(C.asym_grid(kind, L, "row_major", "one")), (kind, L)
    for kw in C.RECT_CHAINS:
        for w in C.RECT_WIDTHS:
            assert C.banded(C.rect_chain(w, **kw)), (kw, w)
    assert all(C.banded(C.ties_grid(L, "row_major")) for L in C.TIE_LABELS)
    assert all(C.banded(C.primal_grid(L, "row_major")) for L in C.PRIMAL_LABELS)
    assert C.banded(C.rtype_grid(M.RTYPE_SHARED)) and C.banded(C.directional_grid()) and C.banded(C.multipass_grid("row_major"))
    assert C.banded(C.rows_mixed_model()) and C.banded(C.mid_grid()) and not C.banded(C.mixed_level_grid())
    fz = [C.banded(C.fuzz_case(s)[0]) for s in range(C.N_FUZZ) if C.fuzz_case(s)[0].has_diff]
    assert 10 < sum(fz) < len(fz) - 10                                  # the family holds both


def test_oracle_runs_every_expansion_of_the_gpu_tests():
    n = 0
    for name, m in C.gpu_expansion_cases():
        n += 1
        x = C.expand(m)
        assert not x.has_diff and not x.has_shared, name
        for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
            o = Oracle(x)
            o.set_reparametrization(mode)
            lb0 = o.LowerBound()
            o.ComputePass(2)
            lb = o.LowerBound()
            assert np.isfinite(lb0) and np.isfinite(lb) and lb >= lb0 - 1e-9 * max(1.0, abs(lb0)), (name, mode, lb0, lb)
            assert not np.any(np.isnan(o.duals())), name
    assert n == C.N_GPU_EXPANSIONS
