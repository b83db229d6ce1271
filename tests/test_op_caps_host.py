"""The op-count caps of the packed kernels and the size limits of the device, host side (the models: tests/op_cap_cases.py; the
device side: tests/test_op_caps_gpu.py).  The caps restated there are those of plan.hpp; the planner splits every case, direction and
mode where they say; the list holds every packed class at 8, 9, cap - 1 and cap ops with cap + 1 moved away (the census); the banded
cases plan as ONE chain launch; dropping the op in a slab's LAST slot changes the oracle's duals, so the device tests on these inputs
would see a kernel that lost it; and a factor past 32767 active receives or sends is refused with the status lpmp_engine.h documents."""
import os
import re

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from oracle.binding import Oracle

import op_cap_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LPMP_ERR_UNSUPPORTED = -2                         # include/lpmp_engine.h


def test_restated_caps_are_those_of_plan_hpp():
    src = open(os.path.join(ROOT, "lp_mp_amd", "csrc", "plan.hpp")).read()
    def const(name):
        (v,) = re.findall(r"constexpr int(?:64_t)? %s = (\d+);" % name, src)
        return int(v)
    for name in ("PK_MAX_OPS", "PW_MAX_OPS", "BIG_MAX_LABELS", "SHARED_MAX_TABLES", "SMALL_MAXD", "MAILBOX_SENDS", "CHAIN_MIN_LAUNCHES"):
        assert const(name) == getattr(OC, name), name
    assert "constexpr int pk_indirect_cap(int labels) { return labels >= 16 ? 32 : labels >= 8 ? 16 : 8; }" in src
    assert "constexpr int pk_dense_cap(int labels) { return labels == 16 ? 64 : pk_indirect_cap(labels); }" in src
    assert OC.INDIRECT_CAP == {w: (32 if w >= 16 else 16 if w >= 8 else 8) for w in OC.WIDTHS}
    assert OC.DENSE_CAP == {w: (64 if w == 16 else OC.INDIRECT_CAP[w]) for w in OC.WIDTHS}
    assert "int16_t n_recv, n_send;" in src and OC.MAX_ACTIVE == 2 ** 15 - 1
    assert OC.PACKED_CLASSES + OC.PAIRWISE_CLASSES == [k for k in E.KCLASS_NAMES if k[:5] in ("dense", "potts", "share") and k != "dense_big"] + OC.PAIRWISE_CLASSES
    assert set(OC.PAIRWISE_CLASSES) | {"pairwise4"} == {k for k in E.KCLASS_NAMES if k.startswith("pairwise")}


def test_the_list_is_what_it_says():
    cs = OC.cases()
    assert {c.family for c in cs} == {"hub_side", "star", "banded", "mixed_chain", "pw_dup"}
    for c in OC.family("hub_side"):
        past = c.name.endswith("past cap")
        assert OC.cap_degrees(c.cap, past) == [d for d in (1, 4, 8, 9, c.cap - 1, c.cap, c.cap, c.cap + 1, 2) if past or d <= c.cap], c.name
        m = c.model()
        deg = OC.cap_degrees(c.cap, past)
        n_a, n_b = len(deg), max(deg)
        assert m.n_factors == n_a + n_b + sum(deg) and np.all(np.bincount(m.m_left[m.m_type == 0], minlength=n_a)[:n_a] == deg), c.name
        if c.kind == "shared":
            assert 1 <= m.n_shared_tables <= OC.SHARED_MAX_TABLES, c.name
    hubs = {c.cls for c in OC.family("hub_side")}
    assert hubs == set(OC.PACKED_CLASSES)
    assert {c.cls for c in OC.family("hub_side") if not c.exact and c.kind != "shared" and c.name.endswith("at cap")} == {k for k in OC.PACKED_CLASSES if "_v" in k}
    assert any("5x7" in c.name for c in OC.family("hub_side"))                         # the rectangular variant
    for c in OC.family("star"):
        m = c.model()
        n_spokes = int(re.search(r"(\d+) spokes", c.name).group(1))
        hub_at = c.name.split("hub ")[1]
        h = OC.hub_position(n_spokes, int(hub_at) if hub_at.isdigit() else hub_at)
        left = np.bincount(m.m_left, minlength=n_spokes + 1)[: n_spokes + 1]
        assert left[h] == n_spokes and np.all(np.delete(left, h) == 1), c.name
    for kind, L in OC.FULL_STARS:
        cap = OC.class_cap(OC.class_of(kind, L))
        for hub_at in ("first", "middle", "last"):
            for n_spokes in (cap - 1, cap, cap + 1):
                OC.case("star %s %d labels %d spokes hub %s" % (kind, L, n_spokes, hub_at))
    assert {(c.kind, int(re.search(r"(\d+) labels", c.name).group(1)), c.n_chain // 2) for c in OC.family("banded")} == set(OC.BANDED)
    assert len(OC.family("pw_dup")) == 4 * 2 * 2
    for name, build in OC.LIMITS.items():
        if "spokes" not in name:
            assert max(build().f_dim0.max(), build().f_dim1.max()) <= OC.BIG_MAX_LABELS, name


_CENSUS = None


def _census():
    global _CENSUS
    if _CENSUS is None:
        _CENSUS = OC.census(OC.cases(), E.Plan)
    return _CENSUS


def test_census_is_complete():
    """a condition on the inputs (op_cap_cases.census_gaps says which): every packed class with 8, 9, cap - 1 and cap ops and with
    cap + 1 moved away; at the cap fewer and more than 4 sends, odd and even receives, an anisotropic and a uniform mode, and a launch
    of two or more records at the cap next to smaller ones; the packed pairwise classes at PW_MAX_OPS; every banded shape with two
    full records inside the chain"""
    cen = _census()
    assert OC.census_gaps(cen) == []
    # and nothing of a packed class runs past its cap
    assert all(ops <= OC.class_cap(k) for k, ops in cen.cells if k in OC.PACKED_CLASSES + OC.PAIRWISE_CLASSES)
    # the run-time-dims classes: records BELOW the cap move with their launch
    for k in OC.PACKED_CLASSES:
        if "_v" in k:
            assert any(ops < OC.class_cap(k) and "dense_big" in to for (b, ops), to in cen.moved.items() if b == k), k


@pytest.mark.parametrize("name", [c.name for c in OC.cases()])
def test_the_planner_splits_every_sweep_at_the_restated_caps(name):
    c = OC.case(name)
    m = c.model()
    p = E.Plan(m)
    for d in OC.DIRECTIONS:
        for mode in OC.MODES:
            s = OC.sweep(p, d, mode)
            info = p.schedule_info(d, mode)
            assert info["n_receives"] == int(s.n_recv.sum()) and info["n_sends"] == int(s.n_send.sum()), (name, d, mode)
            if c.kind == "pairwise":
                want = OC.expected_pairwise_split(c, m, s)
            else:
                want = OC.split(OC.expected_record_classes(c, m, s)[1])
            assert p.schedule_classes(d, mode) == want, (name, d, mode)


def test_the_two_stars_of_the_issue():
    for n_spokes, want in ((64, {"dense16": 65}), (65, {"dense16": 65, "dense_big": 1})):
        p = E.Plan(OC.star(16, "dense", n_spokes, "middle"))
        for d in OC.DIRECTIONS:
            for mode in OC.ANISO_MODES:
                assert p.schedule_classes(d, mode) == want, (n_spokes, d, mode)


@pytest.mark.parametrize("name", [c.name for c in OC.family("banded")])
def test_banded_cases_plan_as_one_chain_launch(name, monkeypatch):
    monkeypatch.delenv("LPMP_NO_MAILBOX", raising=False); monkeypatch.delenv("LPMP_NO_CHAIN", raising=False)
    c = OC.case(name)
    k = c.n_chain // 2
    n = OC.banded_n(k)
    m = c.model()
    assert n >= OC.CHAIN_MIN_LAUNCHES and m.n_factors == n + sum(n - o for o in range(1, k + 1))
    p = E.Plan(m)
    for mode in OC.ANISO_MODES:
        for d in OC.DIRECTIONS:
            s = OC.sweep(p, d, mode)
            full = (s.n_recv == k) & (s.n_send == k)
            assert full.sum() == n - 2 * k >= 2 and s.ops.max() == c.n_chain <= c.cap, (name, d, mode)
            assert (c.n_chain > OC.PK_MAX_OPS), name                                       # the indirect form
            assert p.schedule_classes(d, mode) == {c.cls: n}, (name, d, mode)
            ci = p.chain_info(d, mode)
            assert ci["n_chains"] == 1 and ci["n_tickets"] == n and ci["n_plain_launches"] == 0, (name, d, mode, ci)
            assert k > OC.MAILBOX_SENDS and ci["mailbox_rows"] == 0, (name, d, mode, ci)     # more than 4 sends: completion flags
    # one offset more than the cap holds: the full records leave for the streaming class and the chain is gone
    if c.at_cap:
        q = E.Plan(OC.banded(int(re.search(r"(\d+) labels", name).group(1)), range(1, k + 2), OC.banded_n(k + 1), c.kind))
        cls = q.schedule_classes(M.FORWARD, M.REPAM_ANISOTROPIC)
        assert cls.get("dense_big", 0) >= 2 and q.chain_info(M.FORWARD, M.REPAM_ANISOTROPIC)["n_chains"] == 0, (name, cls)


def test_mixed_chain_changes_its_stride_from_ticket_to_ticket(monkeypatch):
    """one chain launch per sweep with packet levels (8 ops), indirect levels (9 ops) and an indirect level at the cap (16 ops); ONE
    indirect launch keeps the whole chain on completion flags — the mailbox marks live in the packets (plan.hpp, OP_MAILBOX)"""
    monkeypatch.delenv("LPMP_NO_MAILBOX", raising=False); monkeypatch.delenv("LPMP_NO_CHAIN", raising=False)
    (c,) = OC.family("mixed_chain")
    g = OC.MIXED_CHAIN
    p = E.Plan(c.model())
    for mode in OC.ANISO_MODES:
        for d in OC.DIRECTIONS:
            s = OC.sweep(p, d, mode)
            assert {2 * g["k"], 2 * g["k"] + 1, c.cap} <= set(s.ops.tolist()) and s.ops.max() == c.cap and np.sum(s.ops == c.cap) == 1, (d, mode)
            assert np.all(np.bincount(s.level)[1:] == 1)                                   # one record per level: one stride per ticket
            ci = p.chain_info(d, mode)
            assert ci["n_chains"] == 1 and ci["n_tickets"] == g["n"] and ci["n_plain_launches"] == 0 and ci["mailbox_rows"] == 0, (d, mode, ci)
    plain = E.Plan(OC.banded(g["L"], range(1, g["k"] + 1), g["n"])).chain_info(M.FORWARD, M.REPAM_ANISOTROPIC)
    assert plain["n_chains"] == 1 and plain["mailbox_rows"] > 0, plain                      # packets alone: the mailbox


def _at_cap_records(c, m, s):
    """indices (into the sweep) of the records that have exactly cap ops and stay on their class"""
    if c.kind == "pairwise":
        return [i for i, (f, ops) in enumerate(zip(s.factor, s.ops)) if m.f_kind[f] != M.F_VECTOR and ops == OC.PW_MAX_OPS]
    base, final = OC.expected_record_classes(c, m, s)
    return [i for i in range(base.shape[0]) if final[i] == c.cls and s.ops[i] == c.cap]


def _custom_duals(m, rows):
    o = Oracle(OC.oracle_model(m))
    o.compute_pass_custom(*rows)
    return o.duals().copy()


@pytest.mark.parametrize("name", [c.name for c in OC.cases() if c.at_cap])
def test_dropping_the_op_in_the_last_slot_changes_the_duals(name):
    """the plan's own rows of a directional sweep through the oracle, three times: as they are; with the LAST active receive of a record
    at the cap masked out; with its LAST active send's weight set to 0.  A record's ops fill its slab receives first, then sends: a
    kernel that dropped the op in the last slot (or the last receive before the sends) computes one of the other two."""
    c = OC.case(name)
    m = c.model()
    p = E.Plan(m)
    seen = set()
    for mode in OC.MODES:
        for d in OC.DIRECTIONS:
            s = OC.sweep(p, d, mode)
            at = _at_cap_records(c, m, s)
            if not at:
                continue
            i = at[-1]
            oo, om = p.omega(d, mode); mo, mk = p.mask(d, mode)
            what = [w for w, n in (("receive", s.n_recv[i]), ("send", s.n_send[i])) if n > 0 and w not in seen]
            if not what:
                continue
            rows = (s.factor, oo, om, mo, mk)
            plain = _custom_duals(m, rows)
            if "receive" in what:
                mk2 = mk.copy()
                mk2[mo[i] + np.flatnonzero(mk[mo[i]: mo[i + 1]])[-1]] = 0
                assert not np.array_equal(_custom_duals(m, (s.factor, oo, om, mo, mk2)), plain), (name, d, mode, "receive")
            if "send" in what:
                om2 = om.copy()
                om2[oo[i] + np.flatnonzero(om[oo[i]: oo[i + 1]])[-1]] = 0.0
                assert not np.array_equal(_custom_duals(m, (s.factor, oo, om2, mo, mk)), plain), (name, d, mode, "send")
            seen |= set(what)
    assert seen == {"receive", "send"}, (name, seen)


def test_a_factor_past_32767_active_messages_is_refused_as_unsupported():
    """include/lpmp_engine.h: at most 32767 active receives and 32767 active sends per updated factor, LPMP_ERR_UNSUPPORTED when the
    schedules are built (the model is valid in the reference: not LPMP_ERR_INVALID).  lpmp_plan_create takes the model."""
    m = OC.LIMITS["star 2 labels 32767 spokes"]()
    p = E.Plan(m)
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM):
        s = OC.sweep(p, M.FORWARD, mode)
        assert (s.n_recv.max(), s.n_send.max()) == ((OC.MAX_ACTIVE // 2, OC.MAX_ACTIVE // 2 + 1) if mode == M.REPAM_ANISOTROPIC else (OC.MAX_ACTIVE, OC.MAX_ACTIVE))
        assert p.schedule_classes(M.FORWARD, mode) == {"dense_v4": OC.MAX_ACTIVE, "dense_big": 1}, mode
    m = OC.LIMITS["star 2 labels 32768 spokes"]()
    p = E.Plan(m)                                                                      # accepted
    hub = OC.hub_position(OC.MAX_ACTIVE + 1, "middle")
    for d in OC.DIRECTIONS:
        for mode in (M.REPAM_UNIFORM, M.REPAM_DAMPED_UNIFORM):
            with pytest.raises(E.EngineError) as err:
                p.schedule_classes(d, mode)
            assert err.value.code == LPMP_ERR_UNSUPPORTED and "factor %d " % hub in str(err.value) and "32767" in str(err.value), (d, mode, str(err.value))
        # the anisotropic modes split the hub's messages into receives and sends: 16384 of each, within the limit
        assert p.schedule_classes(d, M.REPAM_ANISOTROPIC) == {"dense_v4": OC.MAX_ACTIVE + 1, "dense_big": 1}, d


def test_the_streaming_limits_plan_on_the_streaming_class():
    for name, build in OC.LIMITS.items():
        if "spokes" in name and "40 labels" not in name:
            continue
        m = build()
        p = E.Plan(m)
        n_rec = int(np.sum(m.f_kind == M.F_VECTOR))
        for d in OC.DIRECTIONS:
            for mode in OC.MODES:
                assert p.schedule_classes(d, mode) == {"dense_big": n_rec}, (name, d, mode)
