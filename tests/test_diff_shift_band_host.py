"""The banded form of shifted difference-indexed factors on the host: the numpy statement of the banded receive against the
brute-force minimum over expand_diff()'s table, ``model.diff_shift_band`` against the expanded vector, and the planner's rule —
which launches of class diff with a DIFF_SHIFT factor run sweep_diff_shift_band_kernel (structure and pool values, never a shift)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import diff_shift_band_cases as C                 # noqa: E402
from lp_mp_amd import engine as E                 # noqa: E402
from lp_mp_amd import model as M                  # noqa: E402
from oracle.binding import Oracle                 # noqa: E402

ANISO = M.REPAM_ANISOTROPIC


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ---- the receive --------------------------------------------------------------------------------------------------------------
def test_case_list_has_every_named_placement():
    """the shifts of the case list put the bands where their names say (otherwise the cases below prove less than they claim)"""
    met = set()
    for name, D, d0, d1, s in C.receive_cases():
        lo, hi = M.diff_band(D)
        ne, off = d0 + d1 - 1, d1 - 1 - s
        le, he = M.diff_shift_band(D, d0, d1, s)
        p = name.split()[-1]
        if p == "wholly_left":
            assert (le, he) == (0, -1) and hi + off < 0, name
        elif p == "wholly_right":
            assert (le, he) == (ne, ne - 1) and lo + off > ne - 1, name
        elif p == "clipped_left" and hi - lo >= 1:
            assert le == 0 and lo + off < 0 <= he, name
        elif p == "clipped_right" and hi - lo >= 1:
            assert he == ne - 1 and hi + off > ne - 1 and le <= ne - 1, name
        elif p == "centred" and lo <= hi and hi - lo + 1 <= ne - 2:
            assert 0 < le <= he < ne - 1, name
        elif p == "plain":
            assert s == d1 - 1
        elif p.startswith("huge"):
            assert abs(s) == 1 << 30
        met.add((name.split()[0], p))
    vectors = {"n1", "n2", "constant", "empty_unequal", "unequal", "equal", "long", "zeros", "inf"}
    assert {v for v, _ in met} == vectors and {p for _, p in met} == set(C.PLACEMENTS)
    z = C.named_vectors(3)["zeros"]
    assert np.signbit(z[0]) and not np.signbit(z[-1]) and z[0] == z[-1]          # -0.0 against +0.0: equal values, other bits
    assert M.diff_band(C.named_vectors(3)["empty_unequal"]) == (1, 0)


def test_banded_receive_equals_the_brute_force_minimum_bit_for_bit():
    n_cases = 0
    for name, D, d0, d1, s in C.receive_cases():
        for side in (0, 1):
            oth = d1 if side == 0 else d0
            scales = (1.0, 0.625) if np.all(np.isfinite(D)) else (1.0,)
            for mo in C.other_side_vectors(oth, d0 * 31 + d1):       # random; with ties; zeros of both signs; +inf entries
                for sc in scales:
                    q = C.minplus_shift_banded(D, d0, d1, sc, s, mo, side)
                    ref = C.minplus_expanded(D, d0, d1, sc, s, mo, side)
                    assert _same_bits(q, ref), (name, side, sc, q, ref)
                    n_cases += 1
    assert n_cases > 5000


def test_banded_receive_random_shifts_and_vectors():
    """random vectors with a band anywhere, shifts in +-(n + 14), +inf ends: the rule of the band is not asked (it is exact for any width)"""
    rng = np.random.default_rng(8)
    for _ in range(1500):
        d0, d1, n = int(rng.integers(1, 12)), int(rng.integers(1, 12)), int(rng.integers(1, 14))
        lo = int(rng.integers(0, n + 1))
        w = int(rng.integers(0, n - lo + 1))
        ends = rng.choice([0.5, 2.0, np.inf], 2)
        D = C.window_vector(n, lo, w, ends[0], ends[1], int(rng.integers(1 << 20)))
        s = int(rng.integers(-(n + 14), n + 15))
        side = int(rng.integers(2))
        mo = C.other_side_vectors(d1 if side == 0 else d0, int(rng.integers(1 << 20)))[int(rng.integers(4))]
        assert _same_bits(C.minplus_shift_banded(D, d0, d1, 1.0, s, mo, side), C.minplus_expanded(D, d0, d1, 1.0, s, mo, side)), (D, d0, d1, s, side)


def test_model_diff_shift_band_describes_the_expanded_vector():
    """every entry of the expansion below le has the bits of D[0], every entry above he those of D[n - 1], the entries between are
    D[i - off]; and where both ends of the band of D lie strictly inside the expansion, (le, he) IS diff_band of the expanded vector"""
    n_equal = 0
    for name, D, d0, d1, s in C.receive_cases():
        Ex = C.expanded_vector(D, d0, d1, s)
        ne, off = d0 + d1 - 1, d1 - 1 - s
        lo, hi = M.diff_band(D)
        le, he = M.diff_shift_band(D, d0, d1, s)
        assert 0 <= le <= ne and le - 1 <= he <= ne - 1, name
        assert _same_bits(Ex[:le], np.full(le, D[0])) and _same_bits(Ex[he + 1:], np.full(ne - 1 - he, D[-1])), name
        assert _same_bits(Ex[le:he + 1], D[le - off:he - off + 1]) and (he < le or (lo <= le - off and he - off <= hi)), name
        assert M.diff_shift_is_banded(D, d0, d1) == ((hi - lo + 1) * M.DIFF_BAND_DIV <= ne)
        if lo < D.size and 1 <= lo + off and hi + off <= ne - 2 and lo + off <= ne - 1 and hi + off >= 0:
            assert (le, he) == M.diff_band(Ex), (name, le, he, M.diff_band(Ex))
            n_equal += 1
    assert n_equal > 50
    # the plain DIFF factor is the case n = ne, s = d1 - 1
    D = C.window_vector(13, 4, 3, 1.0, 2.0, 1)
    assert M.diff_shift_band(D, 7, 7, 6) == M.diff_band(D) and M.diff_shift_is_banded(D, 7, 7) == M.diff_band_is_banded(D)


# ---- the planner --------------------------------------------------------------------------------------------------------------
def _info(p, mode=ANISO):
    return [p.diff_shift_band_info(d, mode) for d in (0, 1)]


def _all_banded(p, mode=ANISO):
    return all(i["shift_band_launches"] == i["shift_launches"] > 0 and i["shift_band_receives"] == i["shift_receives"] for i in _info(p, mode))


def _none_banded(p, mode=ANISO):
    return all(i["shift_band_launches"] == 0 and i["shift_band_receives"] == 0 and i["shift_launches"] > 0 for i in _info(p, mode))


def test_rule_at_its_edge():
    """a band of exactly (d0 + d1 - 1) / 4 entries is banded, one more entry is full"""
    for L in (40, 13):
        for extra, want in ((0, True), (1, False)):
            m = C.rule_grid(L, extra)
            assert C.banded(m) == want
            p = E.Plan(m)
            assert (_all_banded(p) if want else _none_banded(p)), (L, extra, _info(p))
            lo, hi = p.diff_shift_bands()[0]
            assert hi - lo + 1 == C.widest(L, L) + extra


def test_every_grid_of_the_gpu_cases_is_banded_in_every_mode():
    for L in C.GRID_LABELS:
        m = C.label_grid(L, "colour_major")
        assert C.banded(m), L
        p = E.Plan(m)
        for mode in C.MODES:
            assert _all_banded(p, mode), (L, mode)
        names, V = C.grid_vectors(L)
        assert p.diff_shift_bands() == {t: M.diff_band(v) for t, v in enumerate(V)}
    placed = {pl for L in C.GRID_LABELS for pl in C.placements_of(L)}
    assert {p for _, p in placed} >= set(C.PLACEMENTS)
    for kw in C.RECT_CHAINS:
        assert C.banded(C.rect_chain(**kw)) and _all_banded(E.Plan(C.rect_chain(**kw))), kw


def test_one_unbanded_vector_makes_the_whole_launch_full():
    m = C.one_unbanded_grid()
    assert not C.banded(m) and M.diff_shift_is_banded(m.shared_table(0).reshape(-1), 40, 40)
    assert _none_banded(E.Plan(m))


def test_plain_and_shifted_peers_in_one_record():
    m = C.mixed_kinds_grid()
    assert np.any(m.f_kind == M.F_PAIRWISE_DIFF) and np.any(m.f_kind == M.F_PAIRWISE_DIFF_SHIFT) and C.banded(m)
    p = E.Plan(m)
    assert _all_banded(p)
    assert all(p.diff_band_info(d, ANISO)["band_launches"] == 0 for d in (0, 1))      # the plain banded kernel runs no shifted launch
    assert p.diff_bands() == {0: M.diff_band(m.shared_table(0).reshape(-1)) + (True,)}
    assert p.diff_shift_bands() == {1: M.diff_band(m.shared_table(1).reshape(-1))}
    # the plain DIFF peer goes by its own rule (n = ne, off = 0): one entry beyond it and the launches are full
    wide = C.mixed_kinds_grid(diff_width=C.widest(24, 24) + 1)
    assert _none_banded(E.Plan(wide))
    assert _all_banded(E.Plan(C.mixed_kinds_grid(diff_width=C.widest(24, 24))))


def test_no_diff_band_switches_the_shifted_form_off_too(monkeypatch):
    monkeypatch.setenv("LPMP_NO_DIFF_BAND", "1")
    for m in (C.compact_grid(), C.mixed_kinds_grid(), C.label_grid(65, "row_major")):
        assert C.banded(m) and _none_banded(E.Plan(m))


def test_shifts_never_change_a_launch():
    m = C.compact_grid()
    p = E.Plan(m)
    want = [(p.schedule_info(d, mode), p.diff_shift_band_info(d, mode), p.schedule_classes(d, mode)) for d in (0, 1) for mode in C.MODES]
    assert _all_banded(p)
    for seed in range(4):
        q = E.Plan(C.with_shifts(m, seed))
        assert [(q.schedule_info(d, mode), q.diff_shift_band_info(d, mode), q.schedule_classes(d, mode)) for d in (0, 1) for mode in C.MODES] == want
    huge = np.where(np.arange(C.n_edges(7, 6)) % 2 == 0, 1 << 30, -(1 << 30))
    assert _all_banded(E.Plan(C.compact_grid(shifts=huge)))


def test_set_shared_pool_flips_banded_full_banded():
    m, banded_a, unbanded, banded_b = C.repool_grid()
    p = E.Plan(m)
    assert _all_banded(p)
    pass_before = p.pass_schedule_info(ANISO)
    for vectors, want in ((unbanded, False), (banded_b, True), (unbanded, False), (banded_a, True)):
        x = C.with_pool(m, vectors)
        assert C.banded(x) == want
        p.set_shared_pool(x.sh_data)
        assert (_all_banded(p) if want else _none_banded(p)), _info(p)
        assert p.diff_shift_bands() == {t: M.diff_band(v) for t, v in enumerate(vectors)}
        assert p.diff_shift_band_info(0, ANISO) == E.Plan(x).diff_shift_band_info(0, ANISO)
        assert p.pass_schedule_info(ANISO) == pass_before


def test_old_queries_are_unmoved():
    for m in (C.compact_grid(), C.label_grid(40, "colour_major"), C.rule_grid(40, 1)):
        p = E.Plan(m)
        assert p.diff_bands() == {}
        lo, hi, banded = (E.C.c_int32(), E.C.c_int32(), E.C.c_int())
        for t in range(m.n_shared_tables):
            assert p.L.lpmp_plan_get_diff_band(p.h, t, E.C.addressof(lo), E.C.addressof(hi), E.C.addressof(banded)) == 0
            assert (lo.value, hi.value, banded.value) == (0, -1, -1)
        for d in (0, 1):
            i = p.diff_band_info(d, ANISO)
            assert i["band_launches"] == 0 and i["band_receives"] == 0 and i["diff_launches"] == p.diff_shift_band_info(d, ANISO)["shift_launches"]


def test_oracle_runs_every_expansion_of_the_gpu_cases():
    """the yardstick itself: a pass over every expansion leaves finite duals and a finite bound (+inf tails included)"""
    for name, m in C.gpu_expansion_cases():
        o = Oracle(C.expand(m))
        o.set_reparametrization(ANISO)
        o.ComputePass(1)
        assert np.isfinite(o.LowerBound()) and not np.any(np.isnan(o.duals())), name


def test_lower_bound_as_summed_is_a_sum():
    x = np.random.default_rng(1).uniform(-1, 1, 700)
    assert abs(C.lower_bound_as_summed(x, 0.5) - (np.sum(x) + 0.5)) < 1e-10
    assert C.lower_bound_as_summed(np.arange(113.0), 1.0) == 1.0 + 112 * 113 / 2


# ---- schedules ----------------------------------------------------------------------------------------------------------------
def test_hazard_checker_runs_clean_on_the_case_models(tmp_path_factory):
    import schedule_hazards as H
    import test_schedule_hazards_host as TH
    lib = H.build_probe(tmp_path_factory.mktemp("schedule_probe_shift_band"))
    failures = []
    models = [("compact", C.compact_grid()), ("mixed kinds", C.mixed_kinds_grid()), ("grid 65", C.label_grid(65, "colour_major")),
              ("rect chain", C.rect_chain(**C.RECT_CHAINS[0])), ("one unbanded", C.one_unbanded_grid())]
    for name, m in models:
        def sweeps_of(o):
            yield from TH._plain_sweeps(o, (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM), True)
        TH._check_model(lib, name, m, sweeps_of, failures=failures)
    assert not failures, "\n".join(failures[:10])
