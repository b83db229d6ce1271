"""The session tests without a GPU (tests/session_cases.py): the generator is deterministic and covers what it claims, the harness
runs end to end with a second shadow in the engine's place and agrees with a straight replay through the plain oracle, and it notices
the defects it is for — engines with one seeded defect each make a session fail at the defective call or the first observation
after it.  A green run of tests/test_session_gpu.py means what these tests make it mean."""
import collections
import dataclasses
import zlib

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from oracle.binding import Oracle

import mixed_precision_cases as MP
import recost_cases as RC
import repool_cases as RP
import session_cases as SC

ALL = SC.sessions() + [("hop", s) for s in SC.HOP_SEEDS]


def _cls(step):
    return SC.OP_CLASS[step[0]]


# ---- determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,seed", ALL)
def test_steps_are_a_pure_function_and_prefixes_replay(cell, seed):
    a, b = SC.steps(cell, seed), SC.steps(cell, seed)
    assert a == b and len(a) > 0
    for k in (1, 7, len(a) // 2):
        assert SC.steps(cell, seed, k) == a[:k]
    if cell != "hop":
        assert len(a) == SC.CELLS[cell]["n"]
        assert SC.steps(cell, seed, len(a) + 25)[:len(a)] == a
    for op, args in a:                                  # small printable arguments only: a step names itself in an error message
        assert op in SC.OP_CLASS and all(isinstance(x, (int, str, bool, type(None))) for x in args), (op, args)


# crc32 of repr(steps(cell, seed)) of every session that was committed before the cells of the path and forest moves and hop route 4
# came (computed on the commits before them): a new op, class or cell must leave the sessions that exist as they are
STEP_DIGESTS = {
    "joined32": {0: 0x701a6554, 1: 0xb27b3ebc, 2: 0xd577a5f8, 3: 0x66ba7427},
    "mixed4": {0: 0x7da306fd, 1: 0x8c2d485a, 2: 0xc3af258a, 3: 0x85e85698, 4: 0x26e2e77c, 5: 0x845003a3},
    "rows": {0: 0x2de26086, 1: 0xe247779e, 2: 0x4abdeaa7, 3: 0xc6d6db41},
    "deep": {0: 0x2dc5e04f, 1: 0xc366597f, 2: 0x1115e9cd, 3: 0x01f3443e},
    "lists": {0: 0x3a7d8a6f, 1: 0x399a6905, 2: 0x32a27a3a, 3: 0x04451d75},
    "diffpool": {0: 0x010f493c, 1: 0xe5fda1cb, 2: 0xa274ea55, 3: 0x7f75df4f},
    "windows": {0: 0xf67cdf6c, 1: 0xbae1e167, 2: 0x02fbd3dd, 3: 0xdac8bae1},
    "hop": {0: 0x904bf48f, 1: 0xe05d07c5, 2: 0x03a8f414, 3: 0x17d52bda},
}


def test_the_sessions_from_before_the_windows_cell_are_unchanged():
    for cell, seeds in STEP_DIGESTS.items():
        assert set(seeds) <= set(SC.HOP_SEEDS if cell == "hop" else SC.CELLS[cell]["seeds"]), cell
        for seed, want in seeds.items():
            assert zlib.crc32(repr(SC.steps(cell, seed)).encode()) == want, (cell, seed)
    assert {c for c, _ in ALL} - set(STEP_DIGESTS) == {"relabel", "relabel_lists", "relabel_windows"} and set(SC.HOP_SEEDS) - set(STEP_DIGESTS["hop"]) == {4}


# ---- coverage: a condition on the generator ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", list(SC.CELLS))
def test_committed_sessions_cover_ops_pairs_and_cost_pairs(cell):
    st, ob, ops = SC.admissible_classes(cell)
    seeds = SC.CELLS[cell]["seeds"]
    n_ops, adjacent, near, kinds = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter()
    for seed in seeds:
        assert SC.CELLS[cell]["n"] >= SC.covering_length(cell, seed), (cell, seed, SC.covering_length(cell, seed))
        s = SC.steps(cell, seed)
        for i, step in enumerate(s):
            n_ops[step[0]] += 1
            if step[0] == "refused":
                kinds[step[1][0]] += 1
            if i + 1 < len(s) and _cls(step) in SC.STATE and _cls(s[i + 1]) in SC.OBSERVING:
                adjacent[(_cls(step), _cls(s[i + 1]))] += 1
            if _cls(step) in SC.COST:
                for j in range(i + 1, min(i + 4, len(s))):
                    if _cls(s[j]) in SC.COST and _cls(s[j]) != _cls(step):
                        near[(_cls(step), _cls(s[j]))] += 1
    print(cell, "seeds", seeds, "length", SC.CELLS[cell]["n"], "| ops", len(ops), "least often", min(n_ops[o] for o in ops),
          "| (state, observing) pairs", len(st) * len(ob), "least often", min(adjacent[(a, b)] for a in st for b in ob),
          "| cost pairs", len([1 for a in SC.COST for b in SC.COST if a != b and a in st and b in st]), "| refusal kinds", dict(kinds))
    assert not [o for o in ops if n_ops[o] < 3], {o: n_ops[o] for o in ops if n_ops[o] < 3}
    assert not [(a, b) for a in st for b in ob if adjacent[(a, b)] < 1]
    cost = [c for c in SC.COST if c in st]
    assert not [(a, b) for a in cost for b in cost if a != b and near[(a, b)] < 1]
    for key in SC.CELLS[cell]["models"]:
        precs = {SC.variant(cell, s)["prec"] for s in seeds}
        want = set().union(*[SC.refusal_kinds(key, p) for p in precs]) | {"destroyed_schedule", "stale_readout"}
        want |= {"stale_window_set"} if SC.props(key)["windows"] else set()
        want |= {"stale_path_set", "stale_forest_set"} if SC.props(key)["relabel"] else set()
        assert want <= set(kinds), want - set(kinds)


def _met_open_batch(cell, seed):
    """(class, stood inside) of every state-changing step that directly follows compute_pass(1) while a batch of passes that ran ahead is
    open (session_cases.SpecSim under the observe plan of the session)"""
    s = SC.steps(cell, seed)
    trace, _ = SC.spec_trace(cell, seed, s)
    return [(_cls(s[i]), trace[i][1]) for i in range(1, len(s))
            if _cls(s[i]) in SC.STATE and s[i - 1] == ("compute_pass", (1,)) and trace[i][0] and not (s[i][0] == "compute_pass" and s[i][1] == (1,))]


def test_every_state_changing_class_meets_an_open_speculative_batch():
    """a call that forgets to settle shows only when a batch is open as it comes: in joined32 every admissible state-changing class
    directly follows single passes with speculation usable, most of them with the caller INSIDE the batch (a roll-back); the hops do
    it on their joined32 leg; the two-engine session of joined32 holds such steps; speculation stays usable for most of a session"""
    st, _, _ = SC.admissible_classes("joined32")
    met = [x for seed in SC.CELLS["joined32"]["seeds"] for x in _met_open_batch("joined32", seed)]
    inside = {c for c, i in met if i}
    print("classes that meet an open batch", collections.Counter(c for c, _ in met), "| inside", sorted(inside))
    assert set(st) <= {c for c, _ in met}, set(st) - {c for c, _ in met}
    assert len(inside) >= len(st) - 2, set(st) - inside
    assert len([1 for c, i in _met_open_batch("joined32", 0) if i]) >= 3           # (the seed of the two-engine test)
    for seed in SC.HOP_SEEDS:
        if "joined32" in SC.HOP_ROUTES[seed]:
            assert len([1 for c, i in _met_open_batch("hop", seed) if i]) >= 2, seed
    for seed in SC.CELLS["joined32"]["seeds"]:
        s = SC.steps("joined32", seed)
        sim, usable = SC.SpecSim(), 0
        for (op, a), chk in zip(s, SC.observe_plan("joined32", seed, s)):
            sim.step(op, a, chk)
            usable += sim.max_depth >= 2 and not sim.timing and sim.persistent and sim.rtype == 0
        assert usable >= 0.7 * len(s), (seed, usable, len(s))


def test_cells_reach_the_state_they_are_about():
    """what can be said without a device: the joined32 model rounds AND keeps the peer-minima form; the deep model is one chain with a
    mailbox; the mixed4 seeds hold every precision once with engine-owned and once with borrowed buffers; hops go small, large, small"""
    p = E.Plan(SC.base_model("joined32"))
    assert SC.props("joined32")["rounds"] and p.pass_rotates(SC.ANISO) and p.peer_minima(SC.ANISO) == (True, "")
    ci = E.Plan(SC.base_model("deep")).chain_info(M.FORWARD, SC.ANISO)
    assert ci["n_chains"] == 1 and ci["mailbox_rows"] > 0
    v = [SC.variant("mixed4", s) for s in SC.CELLS["mixed4"]["seeds"]]
    assert sorted((x["prec"], x["borrowed"]) for x in v) == sorted((p, b) for p in SC.PRECISIONS for b in (False, True))
    assert set(SC.variant("joined32", 1)["env"]) == {"LPMP_ROT_BANDS", "LPMP_CHAIN_CACHE_MB", "LPMP_ROT_EXPLICIT"} and set(SC.variant("joined32", 0)["env"]) == {"LPMP_ROT_BANDS"}
    for route in SC.HOP_ROUTES.values():
        nf = [SC.base_model(k).n_factors for k in route]
        assert len(route) == 4 and nf[0] < nf[1] > nf[2]
    for seed in SC.HOP_SEEDS:
        s = SC.steps("hop", seed)
        ups = [i for i, x in enumerate(s) if x[0] == "upload"]
        assert len(ups) == 4 and all(15 <= b - a - 4 <= (36 if seed < 4 else 48) for a, b in zip(ups, ups[1:]))       # (route 4: its sets and first moves)
        rtype = 0
        for i, (op, a) in enumerate(s):                 # the send rule stays across uploads: SHARED when a model comes that draws no other
            rtype = a[0] if op == "set_reparametrization_type" else rtype
            assert not (op == "upload" and not SC.props(a[0])["mrf"] and rtype != 0), (seed, i)
        for i in ups[1:]:
            # (the window set that comes with a DIFF_SHIFT model and the try of the one before stand first)
            # (... and so do the path and forest sets of a model that admits them, and the tries of those of the model before)
            mine = ("window_set_create", "path_set_create", "forest_set_create")
            stale = ("stale_window_set", "stale_path_set", "stale_forest_set")
            r = [x for x in s[i + 1:i + 9] if x[0] not in mine and not (x[0] == "refused" and x[1][0] in stale)]
            assert r[0] == ("refused", ("stale_readout", r[0][1][1])) and r[1][:1] == ("refused",) and r[1][1][0] == "stale_schedule"
            assert (("refused", ("stale_window_set", 0)) in s[i + 1:i + 6]) == SC.props(s[[u for u in ups if u < i][-1]][1][0])["windows"]
            for kind in ("stale_path_set", "stale_forest_set"):
                assert (("refused", (kind, 0)) in s[i + 1:i + 6]) == SC.props(s[[u for u in ups if u < i][-1]][1][0])["relabel"]


# ---- the windows cell: what its committed steps hold ---------------------------------------------------------------------------
def _moves(cell, seed):
    """(step index, model key, form, label counts of the listed unaries, their deltas, inf) of every move_windows step"""
    key, lists, out = None, {}, []
    for i, (op, a) in enumerate(SC.steps(cell, seed)):
        if op == "upload":
            key, lists = a[0], {}
        elif op == "window_set_create":
            lists[a[0]] = SC.window_list(SC.base_model(key), a[1])
        elif op == "move_windows":
            m = SC.base_model(key)
            f = np.asarray(SC.RO.unaries(m) if lists[a[0]] is None else lists[a[0]])
            out.append((i, key, a[2], m.f_dim0[f], SC.window_deltas(m.f_dim0[f], a[1], a[2]), a[3]))
    return out


def test_window_deltas_and_costs_are_what_the_cell_says():
    for d in (24, 72):
        dims = np.full(42, d)
        named = {0, 1, 2, d - 1, d, d + 7}
        seen, zeros = set(), 0
        for seed in range(40):
            x = SC.window_deltas(dims, seed, "host")
            assert set(np.abs(x).tolist()) <= named | (set(range(64, d)) if d > 64 else set()) and x.any()
            assert SC.MW.has_hazard(dims, x) == (d > 64)
            seen |= set(x.tolist())
            zeros += int(np.sum(x == 0))
            e = SC.window_deltas(dims, seed, "equal")
            assert len(set(e.tolist())) == 1 and abs(int(e[0])) in named - {0}
            assert not SC.window_deltas(dims, seed, "zero").any()
        assert {s * v for s in (1, -1) for v in named} <= seen and 0.4 < zeros / (40 * 42) < 0.6
    # the costs: the session's unaries in the old window; every second row keeps the labels that stay bit for bit
    m = SC.base_model("shift24")
    nominal = m.dual_data + 1.0
    f, delta, co, cn, stride = SC.move_args(m, nominal, None, 4, "device_costs", True)
    off = m.dual_offsets()
    assert stride > 24 and co.shape == cn.shape == (42, stride) and np.isinf(co).any() and np.array_equal(np.isinf(co).sum(1), np.isinf(cn).sum(1))
    for i, u in enumerate(f):
        fin = np.isfinite(co[i, :24])
        assert np.array_equal(co[i, :24][fin], nominal[off[u]:off[u] + 24][fin])
    new = SC.moved_nominal(m, nominal, f, delta, cn)
    assert np.all(np.isfinite(new)) and np.array_equal(new[off[f[1]]:off[f[1]] + 24], cn[1, :24])
    assert SC.move_args(m, nominal, None, 4, "host", False)[2:] == (None, None, None)


def test_windows_sessions_hold_what_the_cell_is_about():
    seeds = SC.CELLS["windows"]["seeds"]
    assert all(SC.props(k)["windows"] and SC.props(k)["shift"] and SC.props(k)["rounds"] and SC.props(k)["pool"] for k in ("shift24", "shift72"))
    assert not any(SC.props(k)["windows"] or SC.props(k)["shift"] for c in STEP_DIGESTS if c not in ("hop", "windows") for k in SC.CELLS[c]["models"])
    forms, infs, next_to = collections.Counter(), 0, collections.Counter()
    run_after, decode_after = 0, 0
    cost_ops = ("set_constants", "upload_costs_warm", "upload_costs_cold", "upload_duals", "zero_pairwise_duals", "upload_shared_pool")
    for seed in seeds:
        s, mv = SC.steps("windows", seed), _moves("windows", seed)
        assert {a[0] for op, a in s if op == "upload"} == {"shift24", "shift72"}, seed
        forms.update(x[2] for x in mv)
        infs += sum(1 for x in mv if x[5] and x[2].endswith("_costs"))
        # a move with both signs in 64 ... 71 on the 72-label model: the in-place hazard of move_windows_cases.deltas
        assert any(k == "shift72" and SC.MW.has_hazard(dims, delta) for _, k, _, dims, delta, _ in mv), seed
        # a cap, not a measurement: the cell cannot pass by not moving
        still = [x for x in mv if x[2] == "zero" or not x[4].any()]
        assert 6 * len(still) <= len(mv), (seed, len(still), len(mv))
        for i in range(len(s) - 1):
            if s[i][0] == "move_windows" and s[i + 1][0] in cost_ops:
                next_to[("move", s[i + 1][0])] += 1
            if s[i + 1][0] == "move_windows" and s[i][0] in cost_ops:
                next_to[(s[i][0], "move")] += 1
        # a prepared schedule made before a move runs after it; a decode and the labels follow a move with no cost change between
        made, moved = {}, []
        for i, (op, a) in enumerate(s):
            if op == "upload":
                made, moved = {}, []
            elif op == "schedule_create":
                made[a[0]] = i
            elif op == "move_windows":
                moved.append(i)
            elif op == "schedule_run":
                run_after += any(made[a[0]] < k for k in moved)
        plan = SC.observe_plan("windows", seed, s)
        assert all(plan[i] for i in moved_all(s))          # the duals are compared behind every move
        for i in moved_all(s):
            quiet = next((j for j in range(i + 1, len(s)) if _cls(s[j]) in SC.COST + ("reupload",)), len(s))
            ops = [s[j][0] for j in range(i + 1, quiet)]
            decode_after += "decode_primal" in ops and "labels" in ops[ops.index("decode_primal"):]
    print("forms", dict(forms), "| inf", infs, "| next to", dict(next_to), "| schedule_run after a move", run_after, "| decode and labels after a move", decode_after)
    assert set(forms) == set(SC.MOVE_FORMS) and infs >= 1
    assert not [x for x in cost_ops if next_to[("move", x)] < 1 or next_to[(x, "move")] < 1], dict(next_to)
    assert run_after >= 1 and decode_after >= 1
    # the rows of the committed set_constants steps and the costs of the committed uploads hold shift 0 and shifts that clamp every index
    shifts = []
    for seed in seeds:
        key = None
        for op, a in SC.steps("windows", seed):
            key = a[0] if op == "upload" else key
            m = SC.base_model(key)
            n_L = np.asarray(m.sh_dim1)[m.f_table] + np.maximum(m.f_dim0, m.f_dim1)
            if op == "set_constants":
                f = RP.listed_subset_shift(m, a[0])
                assert np.all(m.f_kind[f] == M.F_PAIRWISE_DIFF_SHIFT)
                shifts += list(zip(RP.rows_for_shift(m, f, a[0])[:, 1], n_L[f]))
            elif op in ("upload_costs_cold", "upload_costs_warm") or (op == "upload" and a[1] is not None):
                c = SC.model_with_costs(key, a[0] if op != "upload" else a[1], False).const_data.reshape(-1, 2)[:, 1]
                shifts += list(zip(c, n_L[m.f_kind == M.F_PAIRWISE_DIFF_SHIFT]))
    assert all(x == np.trunc(x) and abs(x) <= nl for x, nl in shifts)
    assert any(x == 0 for x, _ in shifts) and any(x == -nl for x, nl in shifts) and any(x == nl for x, nl in shifts)
    assert len({x for x, _ in shifts}) > 100


def moved_all(s):
    return [i for i, (op, _) in enumerate(s) if op == "move_windows"]


def test_numpy_statements_know_diff_shift():
    """decode, energy and beliefs of a DIFF_SHIFT model stated on the kind equal those on expand_diff() bit for bit (the oracle runs on
    the expansion); the shift-aware helpers give integer shifts there and leave every other model as it was"""
    m = SC.model_with_costs("shift24", 5, False)
    shifts = m.const_data.reshape(-1, 2)[:, 1]
    assert np.all(shifts == np.trunc(shifts)) and len(set(shifts.tolist())) > 30 and 0.0 in shifts
    assert all(M.diff_shift_int(x) in (0, 1) for x in RC.recost(SC.base_model("shift24"), 5).const_data.reshape(-1, 2)[:, 1])   # (0.25 + u: the hole)
    o = Oracle(RC.oracle_model(m))
    o.set_reparametrization(SC.ANISO)
    o.ComputePass(2)
    d, x = o.duals(), m.expand_diff()
    assert x.n_factors == m.n_factors and np.array_equal(x.dual_offsets(), m.dual_offsets()) and not x.has_diff
    for direction in (0, 1):
        lab = SC.DC.decode_reference(m, d, o.order(direction), 1)
        assert np.array_equal(lab, SC.DC.decode_reference(x, d, o.order(direction), 1))
        e = SC.DC.energy(RP.with_duals(m, SC.original_unaries(m, d)), lab)
        assert np.isfinite(e) and e == SC.DC.energy(RP.with_duals(x, SC.original_unaries(x, d)), lab)
    u = SC.RO.unaries(m)[::5]
    assert np.array_equal(SC.RO.beliefs_np(m, d, u), SC.RO.beliefs_np(x, d, u))
    for key in ("diff40", "shared32", "mixed4", "lists"):
        b = SC.base_model(key)
        assert np.array_equal(RC.recost_shift(b, 3).const_data, RC.recost(b, 3).const_data)
        f = RP.listed_subset(b, 9)
        assert np.array_equal(RP.listed_subset_shift(b, 9), f) and np.array_equal(RP.rows_for_shift(b, f, 9), RP.rows_for(b, f, 9))


@pytest.mark.parametrize("key", ["joined32", "mixed4", "deep"])
def test_a_rounding_sweep_does_not_depend_on_earlier_labels(key):
    """the shadow takes the labels of a ..._pass_and_primal from an oracle that may have been rebuilt since the labels before were
    made (a decode, an earlier sweep): with time stamps that never repeat every slot is set again by the sweep"""
    m = SC.base_model(key)
    a, b = Oracle(RC.oracle_model(m)), Oracle(RC.oracle_model(m))
    for o in (a, b):
        o.set_reparametrization(SC.ANISO)
    a.ComputePassAndPrimal(1)
    b.ComputePass(1)
    for call in ("ComputeForwardPassAndPrimal", "ComputeBackwardPassAndPrimal"):
        getattr(a, call)(5); getattr(b, call)(5)
        assert np.array_equal(a.duals(), b.duals()) and np.array_equal(a.primal(), b.primal())
        assert not np.any(a.primal()[:, 0] >= m.f_dim0)


# ---- the harness end to end ----------------------------------------------------------------------------------------------------
def straight_replay(session):
    """the duals at the end of a session from ONE walk through the plain oracle and the per-feature numpy statements, without the
    Shadow class: what moves duals or costs, in the order of the steps"""
    raw = o = mode = key = prec = nominal = warm_new = None
    rtype, slots, lists = 0, {}, {}

    def rebuild(duals):
        m = RP.with_duals(raw, duals)
        q = Oracle(MP.oracle_model(m) if prec != "f64" else RC.oracle_model(m))
        q.set_reparametrization_type(rtype)
        if mode is not None:
            q.set_reparametrization(mode)
        return q

    for i, (op, a) in enumerate(session):
        if op == "upload":
            key, prec, mode, slots, lists = a[0], a[2], None, {}, {}
            raw = SC.model_with_costs(key, a[1], prec == "f32")
            nominal, warm_new = raw.dual_data, None
            o = rebuild(raw.dual_data)
        elif op == "set_reparametrization":
            mode = a[0]; o.set_reparametrization(mode)
        elif op == "set_reparametrization_type":
            rtype = a[0]; o.set_reparametrization_type(rtype)
        elif op == "compute_pass":
            o.ComputePass(a[0])
        elif op in ("forward_pass", "backward_pass"):
            o.ComputeForwardPass() if op == "forward_pass" else o.ComputeBackwardPass()
        elif op in ("forward_pass_and_primal", "backward_pass_and_primal", "compute_pass_and_primal"):
            {"f": o.ComputeForwardPassAndPrimal, "b": o.ComputeBackwardPassAndPrimal, "c": o.ComputePassAndPrimal}[op[0]](a[0])
        elif op == "compute_pass_custom":
            o.compute_pass_custom(*SC.custom_rows(key, a[0]))
        elif op == "schedule_create":
            slots[a[0]] = SC.custom_rows(key, a[1])
        elif op == "schedule_run":
            o.compute_pass_custom(*slots[a[0]])
        elif op == "upload_costs_cold":
            new = SC.model_with_costs(key, a[0], prec == "f32")
            raw = dataclasses.replace(raw, const_data=new.const_data, _keep=[])
            nominal = new.dual_data
            o = rebuild(new.dual_data)
        elif op == "upload_costs_warm":
            new = SC.model_with_costs(key, a[0], prec == "f32")
            raw = dataclasses.replace(raw, const_data=new.const_data, _keep=[])
            warm_new = new.dual_data
            o = rebuild(o.duals())
        elif op == "set_vectors_diff":
            d, vm = o.duals(), RC.vector_mask(raw)
            d[vm] = d[vm] + (warm_new[vm] - nominal[vm])
            nominal = warm_new
            o = rebuild(d)
        elif op == "set_vectors":
            f, rows = SC.vector_subset(raw, a[0])
            o = rebuild(RC.scatter_rows(raw, o.duals(), f, rows, a[1]))
        elif op == "zero_pairwise_duals":
            o = rebuild(RC.zero_pairwise(raw, o.duals()))
        elif op == "set_constants":
            f = RP.listed_subset_shift(raw, a[0])
            raw = RP.with_rows(raw, f, RP.rows_for_shift(raw, f, a[0], float_valued=prec == "f32"))
            o = rebuild(o.duals())
        elif op == "window_set_create":
            lists[a[0]] = SC.window_list(raw, a[1])
        elif op == "move_windows":
            f, delta, co, cn, _ = SC.move_args(raw, nominal, lists[a[0]], a[1], a[2], a[3])
            raw, d = M.move_windows(raw, o.duals(), f, delta, co, cn)
            nominal = SC.moved_nominal(raw, nominal, f, delta, cn)
            warm_new = None if warm_new is None else SC.moved_nominal(raw, warm_new, f, delta)
            o = rebuild(d)
        elif op == "upload_shared_pool":
            raw = raw.with_pool(SC.pool_variant(raw, a[0]))
            o = rebuild(o.duals())
        elif op == "upload_duals":
            o = rebuild(o.duals() * 0.5)
    return o.duals(), o.LowerBound()


@pytest.mark.parametrize("cell,seed", ALL)
def test_sessions_run_with_a_second_shadow_in_the_engines_place(cell, seed):
    session = SC.steps(cell, seed)
    shadow = SC.Shadow()
    SC.run(SC.Shadow(), shadow, session, observe=SC.observe_plan(cell, seed, session), cell=cell, seed=seed)
    duals, lb = straight_replay(session)
    assert np.array_equal(shadow.download_duals(), duals)
    assert shadow.lower_bound() == lb and np.isfinite(lb)


# ---- the harness notices what it is for ----------------------------------------------------------------------------------------
class BoundCachedAcrossSetVectors(SC.Shadow):
    """the next lower_bound after a set_vectors answers with the sum from before it (the listed bounds were not marked stale)"""
    _lb = None

    def set_vectors(self, factors, src, accumulate=False):
        lb = SC.Shadow.lower_bound(self)
        super().set_vectors(factors, src, accumulate)
        self._lb = lb

    def lower_bound(self):
        self._model()
        lb, self._lb = self._lb, None
        return lb if lb is not None else super().lower_bound()


class WarmStartDropsTheDifference(SC.Shadow):
    _warm = False

    def upload_costs(self, const=None, duals=None):
        super().upload_costs(const, duals)
        self._warm = duals is None

    def set_vectors(self, factors, src, accumulate=False):
        if self._warm and accumulate:
            self._warm = False
            return
        super().set_vectors(factors, src, accumulate)


class LabelsSurviveACostChange(SC.Shadow):
    def _keeping(self, call, *a):
        lab = self.labels
        call(*a)
        self.labels = lab

    def upload_costs(self, const=None, duals=None):
        self._keeping(super().upload_costs, const, duals)

    def set_constants(self, factors, src):
        self._keeping(super().set_constants, factors, src)

    def upload_shared_pool(self, sh_data=None):
        self._keeping(super().upload_shared_pool, sh_data)


class RefusedPoolWritesHalf(SC.Shadow):
    def upload_shared_pool(self, sh_data=None):
        try:
            super().upload_shared_pool(sh_data)
        except E.EngineError:
            if sh_data is not None and self.raw.sh_data is not None:
                sh = self.raw.sh_data.copy()
                h = sh.shape[0] // 2
                sh[:h] = np.asarray(sh_data)[:h]
                self.raw = self.raw.with_pool(sh)
                self._rebuild(self.duals())
            raise


class PassAfterModeChangeRunsOldWeights(SC.Shadow):
    """the first compute_pass after a change of mode still runs the weights of the mode before (the directional sweeps do not)"""
    _old = None

    def set_reparametrization(self, mode):
        if self.mode is None or self.mode == int(mode):
            return super().set_reparametrization(mode)
        self._old = self.mode if self._old is None else self._old
        self.mode = int(mode)
        self.o.set_reparametrization(self._old)

    def _rebuild(self, duals):
        super()._rebuild(duals)
        if self._old is not None:
            self.o.set_reparametrization(self._old)

    def upload(self, model, **kw):
        self._old = None
        super().upload(model, **kw)

    def _sync(self):
        if self._old is not None:
            self._old = None
            self.o.set_reparametrization(self.mode)

    def compute_pass(self, n=1):
        super().compute_pass(n)
        self._sync()

    def forward_pass(self): self._sync(); super().forward_pass()
    def backward_pass(self): self._sync(); super().backward_pass()
    def _primal(self, call, it): self._sync(); super()._primal(call, it)


class ZeroSkippedWhileAScheduleExists(SC.Shadow):
    def zero_pairwise_duals(self):
        if any(s is not None for s in self.schedules):
            return
        super().zero_pairwise_duals()


class _StaleReadout(SC.ShadowReadout):
    def vectors(self):
        self._enter()
        return SC.RO.vectors_np(self.sh.raw, self.sh.at_upload, self.factors)

    def beliefs(self):
        self._enter()
        return SC.RO.beliefs_np(self.sh.eff(), self.sh.at_upload, self.factors)


class ReadoutAnswersFromTheUpload(SC.Shadow):
    def upload(self, model, **kw):
        super().upload(model, **kw)
        self.at_upload = np.array(model.dual_data, np.float64, copy=True)

    def readout(self, factors=None):
        return _StaleReadout(self, factors)


# ---- defects of a move (the windows cell) ----
class MoveLeavesTheShifts(SC.Shadow):
    """duals moved, constants kept"""

    def _move(self, ws, delta, cost_old, cost_new):
        raw = self.raw
        super()._move(ws, delta, cost_old, cost_new)
        d, self.raw = self.duals(), raw
        self._rebuild(d)


class MoveSkipsTheMessages(SC.Shadow):
    """theta and shifts moved, message vectors kept"""

    def _move(self, ws, delta, cost_old, cost_new):
        before = self.duals()
        super()._move(ws, delta, cost_old, cost_new)
        d, pw = self.duals(), ~RC.vector_mask(self.raw)
        d[pw] = before[pw]
        self._rebuild(d)


class BoundCachedAcrossAMove(SC.Shadow):
    """the next lower_bound after a move answers with the sum from before it (the bounds were not marked stale)"""
    _lb = None

    def _move(self, ws, delta, cost_old, cost_new):
        lb = SC.Shadow.lower_bound(self)
        super()._move(ws, delta, cost_old, cost_new)
        self._lb = lb

    def lower_bound(self):
        self._model()
        lb, self._lb = self._lb, None
        return lb if lb is not None else super().lower_bound()


class LabelsSurviveAMove(SC.Shadow):
    def _move(self, ws, delta, cost_old, cost_new):
        lab = self.labels
        super()._move(ws, delta, cost_old, cost_new)
        self.labels = lab


class MoveWritesOnlyOnePlace(SC.Shadow):
    """the new shifts reach the packed constants and not the cells the kernels read: modelled as "the next call that gives duals and
    no constants runs on the shifts from before the move" (a call that gives constants writes both places again)"""
    _old = None

    def _move(self, ws, delta, cost_old, cost_new):
        old = self.raw.const_data if self._old is None else self._old
        super()._move(ws, delta, cost_old, cost_new)
        self._old = old

    def _drop(self):
        if self._old is not None:
            self.raw, self._old = dataclasses.replace(self.raw, const_data=self._old, _keep=[]), None

    def upload_duals(self, d):
        self._drop(); super().upload_duals(d)

    def zero_pairwise_duals(self):
        self._drop(); super().zero_pairwise_duals()

    def upload_costs(self, const=None, duals=None):
        self._old = None if const is not None else self._old
        self._drop(); super().upload_costs(const, duals)

    def set_constants(self, factors, src):
        self._old = None; super().set_constants(factors, src)

    def upload(self, model, **kw):
        self._old = None; super().upload(model, **kw)


class StaleSetStillMoves(SC.Shadow):
    def _window_set_alive(self, ws):
        return self.raw is not None


_PASSES = ("compute_pass", "forward_pass", "backward_pass", "compute_pass_custom", "schedule_run", "forward_pass_and_primal",
           "backward_pass_and_primal", "compute_pass_and_primal")
_COSTS_SEEN = ("lower_bound", "factor_lower_bounds", "ro_beliefs", "refused") + _PASSES
# defect of a move -> (ops whose call is defective, ops that show it whenever the call before bit, ops that may show it, forms of a
# move that cannot bite)
MOVE_DEFECTS = {
    MoveLeavesTheShifts: (("move_windows",), _COSTS_SEEN, ("labels", "decode_primal"), ("zero", "equal")),
    MoveSkipsTheMessages: (("move_windows",), (), (), ("zero",)),
    BoundCachedAcrossAMove: (("move_windows",), ("lower_bound",), (), ("zero",)),
    LabelsSurviveAMove: (("move_windows",), (), ("labels", "ro_labels"), ()),
    MoveWritesOnlyOnePlace: (("upload_duals", "zero_pairwise_duals"), _COSTS_SEEN, ("labels", "decode_primal"), ("zero", "equal")),
    StaleSetStillMoves: (("refused",), (), (), ()),
}


@pytest.mark.parametrize("defect", list(MOVE_DEFECTS), ids=lambda d: d.__name__)
def test_a_seeded_defect_of_a_move_fails_the_windows_session_where_it_is(defect):
    """the first committed session of the windows cell fails: at the defective call, or at the first observation behind a defective
    call that bit (a move of a form that changes what the defect leaves out) which can show it"""
    at, shows, may, idle = MOVE_DEFECTS[defect]
    seed = SC.CELLS["windows"]["seeds"][0]
    session = SC.steps("windows", seed)
    with pytest.raises(SC.Mismatch) as ei:
        SC.run(defect(), SC.Shadow(), session, observe=None, cell="windows", seed=seed)
    i, msg = ei.value.index, str(ei.value)
    print(defect.__name__, "noticed at step", i, session[i])
    assert ("session windows seed %d, step %d %s" % (seed, i, session[i][0])) in msg and "the last steps:" in msg
    if defect is StaleSetStillMoves:
        assert session[i][0] == "refused" and session[i][1][0] == "stale_window_set" and "expected -4, got no error" in msg
        assert i == next(k for k, x in enumerate(session) if x[:1] + x[1][:1] == ("refused", "stale_window_set"))
        return
    if defect is MoveSkipsTheMessages:
        # the very first move that moves anything while a message is not zero (every step's duals are compared: observe=None)
        assert session[i][0] == "move_windows" and "duals: first difference" in msg
        first = next(k for k, (op, a) in enumerate(session) if op == "move_windows" and a[2] != "zero")
        assert i == first and any(op in _PASSES for op, _ in session[:i])
        return
    bit = [k for k in range(i) if session[k][0] == "move_windows" and session[k][1][2] not in idle]
    assert bit and session[i][0] in at + shows + may, (i, session[i])
    if defect is LabelsSurviveAMove:                     # (labels that were unset when the windows moved show nothing)
        return
    if defect is MoveWritesOnlyOnePlace:
        drops = [k for k in range(bit[0], i + 1) if session[k][0] in at]
        assert drops and not [k for k in range(drops[0] + 1, i) if session[k][0] in shows], (drops, i)
        return
    # nothing that shows it whenever it bit stands between the first move that bit and the step that noticed
    assert not [k for k in range(bit[0] + 1, i) if session[k][0] in shows], (bit[0], i)


# defect -> (ops whose call is defective, ops that may be the first to show it)
DEFECTS = {
    BoundCachedAcrossSetVectors: (("set_vectors", "set_vectors_diff"), ("lower_bound",)),
    WarmStartDropsTheDifference: (("set_vectors_diff", "set_vectors"), ()),
    LabelsSurviveACostChange: (("upload_costs_cold", "upload_costs_warm", "set_constants", "upload_shared_pool"), ("labels", "ro_labels")),
    RefusedPoolWritesHalf: (("refused",), ()),
    PassAfterModeChangeRunsOldWeights: (("compute_pass",), ()),
    ZeroSkippedWhileAScheduleExists: (("zero_pairwise_duals",), ()),
    ReadoutAnswersFromTheUpload: (("upload", "compute_pass", "forward_pass", "backward_pass", "set_vectors", "upload_duals", "schedule_run",
                                   "compute_pass_custom", "upload_costs_cold", "set_vectors_diff", "zero_pairwise_duals",
                                   "forward_pass_and_primal", "backward_pass_and_primal", "compute_pass_and_primal"), ("ro_vectors", "ro_beliefs")),
}


def _admissible(defect, cell):
    p = [SC.props(k) for k in SC.CELLS[cell]["models"]]
    if defect is RefusedPoolWritesHalf:
        return all(x["pool"] for x in p)
    if defect is LabelsSurviveACostChange:
        return all(x["mrf"] for x in p)                 # (a model the rounding code refuses never holds a label)
    return True


def _may_show(defect, session):
    """cheap conditions on the steps without which the defect cannot show in this session"""
    if defect is RefusedPoolWritesHalf:
        return any(x == "refused" and a[0] == "pool_nan" for x, a in session)
    if defect is ZeroSkippedWhileAScheduleExists:
        live = set()
        for x, a in session:
            if x == "upload":
                live = set()
            elif x == "schedule_create":
                live.add(a[0])
            elif x == "schedule_destroy":
                live.discard(a[0])
            elif x == "zero_pairwise_duals" and live:
                return True
        return False
    return True


@pytest.mark.parametrize("cell", list(SC.CELLS))
@pytest.mark.parametrize("defect", list(DEFECTS), ids=lambda d: d.__name__)
def test_a_seeded_defect_fails_the_session_where_it_is(defect, cell):
    """the first committed session of the cell in which the defect can show fails, at the defective call or at the first observation
    after it that can show it"""
    if not _admissible(defect, cell):
        return
    at, shows = DEFECTS[defect]
    for seed in SC.CELLS[cell]["seeds"]:
        session = SC.steps(cell, seed)
        if not _may_show(defect, session):
            continue
        try:
            SC.run(defect(), SC.Shadow(), session, observe=None, cell=cell, seed=seed)
        except SC.Mismatch as ex:
            i, msg = ex.index, str(ex)
            break
    else:
        pytest.fail("no committed session of %s notices %s" % (cell, defect.__name__))
    print(defect.__name__, cell, "seed", seed, "noticed at step", i, session[i])
    assert ("session %s seed %d, step %d %s" % (cell, seed, i, session[i][0])) in msg and "the last steps:" in msg and ("difference at" in msg or " / " in msg)
    if session[i][0] in at:
        return                                          # the defective call itself
    # ... or the first observation after a defective call that can show it (the comparison after the last step included)
    assert session[i][0] in shows or i == len(session) - 1, (i, session[i])
    before = [k for k in range(i) if session[k][0] in at]
    assert before, (i, session[i])
    if defect is not LabelsSurviveACostChange:           # (labels that were unset when the costs changed show nothing)
        assert not [k for k in range(before[-1] + 1, i) if session[k][0] in shows], (before[-1], i)


@pytest.mark.parametrize("cell", ["diffpool", "mixed4", "deep", "hop", "windows", "relabel", "relabel_windows"])
def test_replay_with_a_fresh_engine_in_the_middle(cell):
    """tests/session_replay.py --fresh-at K: a new engine takes over with the shadow's model, duals, mode, read-outs, schedules and
    labels — K right behind a step that sets labels which a later step still observes (no cost change in between unsets them).  The
    cells of the path and forest moves: K right behind a move, and the engine that takes over moves on a set it made again from the
    shadow's lists"""
    unsets = ("upload", "upload_costs_cold", "upload_costs_warm", "set_constants", "upload_shared_pool", "move_windows")
    moves = ("path_moves", "forest_moves")
    relabel = cell.startswith("relabel")
    k = None
    for seed in (SC.HOP_SEEDS if cell == "hop" else SC.CELLS[cell]["seeds"]):
        s = SC.steps(cell, seed)
        for i in [i for i, (op, a) in enumerate(s) if (op in moves if relabel else op == "decode_primal" or op.endswith("_and_primal"))]:
            j = next((j for j in range(i + 1, len(s)) if s[j][0] in ("labels", "ro_labels") or s[j][0] in unsets), None)
            if j is not None and s[j][0] not in unsets:
                k = i + 1
                break
        if k is not None:
            break
    assert k is not None
    if relabel:
        made = {a[0] for op, a in s[:k] if op.endswith("_set_create")}
        upto = next((j for j in range(k, len(s)) if s[j][0] == "upload"), len(s))
        assert [j for j in range(k, upto) if s[j][0] in moves and s[j][1][0] in made], (cell, seed, k)
    SC.run([SC.Shadow()], SC.Shadow(), s, observe=None, cell=cell, seed=seed, fresh_at=k, fresh=SC.Shadow)


# ---- the cells of the path and forest moves: what their committed steps hold ------------------------------------------------------
RELABEL_CELLS = ("relabel", "relabel_lists", "relabel_windows")
_LIST_TEXT = {"path_set_ring": "non-consecutive members of path 0", "path_set_neighbours_in_group": "two paths of group 0",
              "forest_set_not_induced": "induce a forest", "forest_set_no_edge": "no pairwise factor joins"}


def _relabel_sessions():
    return [(c, s) for c in RELABEL_CELLS for s in SC.CELLS[c]["seeds"]] + [("hop", 4)]


def test_committed_path_and_forest_lists_are_legal_and_the_refusal_lists_are_refused():
    """every list of a committed path_set_create / forest_set_create step is accepted by Plan.path_info / Plan.forest_info on the
    model of the step; every refusal list is refused by them with the code of the header and the text the kind is about.  The
    chains of rrows — one per tree of each suggested forest group — are legal path groups"""
    forms, n_lists = collections.Counter(), 0
    for cell, seed in _relabel_sessions():
        key = None
        for op, a in SC.steps(cell, seed):
            key = a[0] if op == "upload" else key
            if op == "path_set_create":
                info = SC.structure_plan(key).path_info(SC.path_list(key, a[1]))
                assert info["n_paths"] >= 1, (cell, seed, op, a)
                forms[(key, a[1] % 4)] += 1
                n_lists += 1
            elif op == "forest_set_create":
                info = SC.structure_plan(key).forest_info(SC.forest_list(key, a[1]))
                assert info["n_trees"] >= 1, (cell, seed, op, a)
                forms[(key, "cover" if a[1] is None else "seeded")] += 1
                n_lists += 1
    print("lists", n_lists, dict(forms))
    assert {f for _, f in forms} == {0, 1, 2, 3, "cover", "seeded"}
    for key in SC.RELABEL_GRIDS:
        have = {f for k, f in forms if k == key}
        assert have & {0, 1, 2, 3} and have & {"cover", "seeded"}, (key, have)
        for kind, text in _LIST_TEXT.items():
            lst = SC.refusal_list(key, kind)
            with pytest.raises(E.EngineError) as ei:
                (SC.structure_plan(key).path_info if kind.startswith("path") else SC.structure_plan(key).forest_info)(lst)
            assert ei.value.code == SC.ERR_INVALID and text in str(ei.value), (key, kind, str(ei.value))
    chains = SC.cover_chains(SC.suggested_cover("rrows"))
    info = SC.structure_plan("rrows").path_info(chains)
    assert info["n_paths"] == sum(int(np.sum(par == -1)) for _, par in SC.suggested_cover("rrows")) and info["n_path_edges"] > info["n_paths"]
    # the grid of rlists is the first factors of the model, and nothing else of it is eligible for a move
    assert max(int(u.max()) for u, _ in SC.suggested_cover("rlists")) < 20 and not SC.props("rlists")["mrf"]
    # 8, 24 and 72 labels: the lane-group, wave and workgroup forms; rmixed4 holds SHARED, DIFF and Potts links
    assert [int(SC.base_model(k).f_dim0.max()) for k in ("rgrid8", "rshift24", "rshift72")] == [8, 24, 72]
    kinds = set(SC.base_model("rmixed4").f_kind.tolist())
    assert {M.F_PAIRWISE_SHARED, M.F_PAIRWISE_DIFF, M.F_PAIRWISE_POTTS, M.F_PAIRWISE_DENSE} <= kinds


def _count(cell, pattern):
    """how often the committed sessions of the cell hold these ops as neighbours ("mv": a path or forest move of one round at least;
    "same": such a move on the set of the "mv" / the create before it)"""
    n = 0
    for seed in SC.CELLS[cell]["seeds"]:
        s = SC.steps(cell, seed)
        for i in range(len(s) - len(pattern) + 1):
            slot, ok = None, True
            for (op, a), want in zip(s[i:], pattern):
                if want in ("mv", "same"):
                    ok = op in ("path_moves", "forest_moves") and a[1] > 0 and (want == "mv" or a[0] == slot)
                else:
                    ok = op == want
                if not ok:
                    break
                slot = a[0] if want == "mv" or want.endswith("_set_create") else slot
            n += ok
    return n


def test_relabel_sessions_hold_what_their_cells_are_about():
    cost_ops = ("upload_costs_cold", "upload_costs_warm", "set_constants", "upload_shared_pool", "move_windows")
    moves = ("path_moves", "forest_moves")
    for cell in RELABEL_CELLS:
        behind, rounds, forms, precs, keys = collections.Counter(), collections.Counter(), collections.Counter(), set(), set()
        for seed in SC.CELLS[cell]["seeds"]:
            s = SC.steps(cell, seed)
            plan = SC.observe_plan(cell, seed, s)
            precs.add(SC.variant(cell, seed)["prec"])
            made_before_window_move = 0
            sets_then = set()
            live = set()
            for i, (op, a) in enumerate(s):
                if op == "upload":
                    keys.add(a[0]); live, sets_then = set(), set()
                if op.endswith("_set_create"):
                    live.add(a[0])
                if op == "move_windows":
                    sets_then = set(live)
                if op in moves:
                    assert plan[i], (cell, seed, i)           # the duals are compared behind every move
                    rounds[a[1]] += 1
                    made_before_window_move += a[0] in sets_then
                    nxt = s[i + 1:i + 3]
                    if len(nxt) == 2 and nxt[1][0] in ("labels", "ro_labels"):
                        behind[nxt[0][0] if nxt[0][0] != "refused" else nxt[0][1][0]] += 1
                if op == "upload_primal":
                    forms[a[1]] += 1
            if cell == "relabel_windows":
                assert made_before_window_move >= 1, (cell, seed)
        print(cell, "| behind a move, labels next:", dict(behind), "| rounds", dict(rounds), "| forms", dict(forms), "| keys", sorted(keys))
        assert keys == set(SC.CELLS[cell]["models"]) and set(rounds) == {0, 1, 2, 3}
        st, _, _ = SC.admissible_classes(cell)
        for c in [c for c in SC.COST if c in st]:
            assert any(behind[o] for o in SC.CLASS_OPS[c] if o in cost_ops + ("set_vectors", "set_vectors_diff", "zero_pairwise_duals", "upload_duals")), (cell, c)
        if cell == "relabel_lists":
            # a cost change and each new refusal kind directly behind a move, ro_labels behind it
            assert any(behind[o] for o in cost_ops) and all(behind[k] >= 1 for k in ("labels_lists", "upload_primal_lists", "primal_pass_lists", "decode_lists")), dict(behind)
            assert behind["labels_lists"] >= 3
        else:
            assert set(forms) == set(SC.PRIMAL_FORMS)
            # the fixed blocks: a decode, a move, the labels; a rounding sweep, a move, the labels, a rounding sweep, the labels; a move,
            # a pass, a move on the same set, the labels; a bound, a move, a directional sweep, a bound
            assert _count(cell, ("decode_primal", "mv", "labels")) >= 1
            assert _count(cell, ("compute_pass_and_primal", "mv", "labels", "compute_pass_and_primal", "labels")) >= 1
            assert _count(cell, ("lower_bound", "mv", "forward_pass", "lower_bound")) >= 1
            assert _count(cell, ("upload_primal", "mv", "labels")) >= 3
        assert _count(cell, ("mv", "compute_pass", "same", "labels" if cell != "relabel_lists" else "ro_labels")) >= 1
        if cell == "relabel_windows":
            assert _count(cell, ("path_set_create", "move_windows", "same", "labels")) >= 1 and _count(cell, ("forest_set_create", "move_windows", "same", "labels")) >= 1
        if cell == "relabel":
            assert precs == set(SC.PRECISIONS) and SC.props("rrows")["rows_layout"]
    # the primal arrays: about a third of the unaries unset / stray, the pairwise slots copies of what is below the dimension
    m = SC.base_model("rgrid8")
    un = m.f_kind == M.F_VECTOR
    for form in SC.PRIMAL_FORMS:
        pr = SC.primal_for(m, 5, form)
        unset, stray = pr[un, 0] >= m.f_dim0[un], pr[un, 0] < 0
        assert (0.15 < unset.mean() < 0.5) == (form == "partly_unset") and (0.15 < stray.mean() < 0.5) == (form == "stray")
        assert unset.any() == (form == "partly_unset") and stray.any() == (form == "stray")
    # new costs of rgrid8 tie: a quarter grid
    c = SC.model_with_costs("rgrid8", 7, False)
    assert np.array_equal(c.const_data * 4, np.round(c.const_data * 4)) and np.array_equal(c.dual_data * 4, np.round(c.dual_data * 4))
    assert len(np.unique(c.const_data)) <= 5


# ---- defects of the path and forest moves and of the labels they leave -------------------------------------------------------------
class CostChangeLeavesMovedLabelsOnLists(SC.Shadow):
    """(a) on a model the rounding code refuses a change of costs leaves the labels a move wrote"""

    def _keeping(self, call, *a):
        lab = self.labels
        call(*a)
        if not self._mrf():
            self.labels = lab

    def upload_costs(self, const=None, duals=None):
        self._keeping(super().upload_costs, const, duals)

    def set_constants(self, factors, src):
        self._keeping(super().set_constants, factors, src)

    def upload_shared_pool(self, sh_data=None):
        self._keeping(super().upload_shared_pool, sh_data)


class RefusedLabelCallUnsetsLists(SC.Shadow):
    """(b) on such a model a refused call that asks for the rounding tables frees the array the move wrote into"""

    def _rounding_tables(self):
        try:
            super()._rounding_tables()
        except E.EngineError:
            if self.raw is not None:
                self.labels = SC.unset_labels(self.raw)
            raise

    def _primal(self, call, it):
        self._mode()
        self._rounding_tables()
        super()._primal(call, it)


class MoveTakesTheLastMinimiser(SC.Shadow):
    """(c)"""

    def _reference(self, m, d, lab, ms, rounds):
        groups = ms.groups if ms.kind == "forest" else M.forests_from_paths(ms.groups)
        return SC.FM.forest_moves_reference(m, d, lab, groups, rounds, variant="last")


def _members(ms):
    return sorted({int(u) for g in ms.groups for p in g for u in p} if ms.kind == "path" else {int(u) for un, _ in ms.groups for u in un})


def _with_other_labels(sh, m, d, lab, ms, rounds, change):
    """the move on an array in which ``change`` rewrote the unary labels; unaries that are in no group keep what they held"""
    if rounds == 0 or not _members(ms):
        return lab.copy()
    lab2 = lab.copy()
    change(lab2)
    new = SC.Shadow._reference(sh, m, d, lab2, ms, rounds)
    off = np.setdiff1d(np.flatnonzero(m.f_kind == M.F_VECTOR), _members(ms))
    new[off, 0] = lab[off, 0]
    return SC.PM.propagate(m, new, SC.PM.structure(m)[1])


class MoveIgnoresOffListNeighbours(SC.Shadow):
    """(d) a unary that is in no group of the set counts with label 0"""

    def _reference(self, m, d, lab, ms, rounds):
        def change(x):
            x[np.setdiff1d(np.flatnonzero(m.f_kind == M.F_VECTOR), _members(ms)), 0] = 0
        return _with_other_labels(self, m, d, lab, ms, rounds, change)


class MoveReadsTheDualsBeforeTheLastPass(SC.Shadow):
    """(e) a move reads the message vectors of the pairwise factors as they were before the most recent pass (rows that were not
    refreshed) next to the unaries of the moment.  (With ALL duals from before the pass a move would see the same energy, up to
    rounding: theta_u + sum m_s is the original unary under every reparametrisation)"""
    _old = None

    def _rebuild(self, duals):
        self._old = None
        super()._rebuild(duals)

    def compute_pass(self, n=1):
        old = self.duals()
        super().compute_pass(n)
        self._old = old

    def _reference(self, m, d, lab, ms, rounds):
        if self._old is not None:
            pw = ~RC.vector_mask(m)
            d = np.array(d, np.float64, copy=True)
            d[pw] = self._old[:len(d)][pw]
        return super()._reference(m, d, lab, ms, rounds)


class MoveSkipsThePairwiseSlots(SC.Shadow):
    """(f)"""

    def _relabel(self, ms, rounds):
        before = self.labels.copy()
        super()._relabel(ms, rounds)
        pw = self.raw.f_kind != M.F_VECTOR
        self.labels[pw] = before[pw]


class StaleMoveSetStillMoves(SC.Shadow):
    """(g) a set survives an upload"""

    def _move_set_alive(self, ms):
        return self.raw is not None

    def _relabel(self, ms, rounds):
        if ms.gen == self.gen:
            super()._relabel(ms, rounds)


class UnsetNeighbourCountsAsLabelZero(SC.Shadow):
    """(h) a unary without a label counts with label 0, not with its last label"""

    def _reference(self, m, d, lab, ms, rounds):
        def change(x):
            un = np.flatnonzero(m.f_kind == M.F_VECTOR)
            x[un, 0] = np.where(x[un, 0] >= m.f_dim0[un], 0, x[un, 0])
        return _with_other_labels(self, m, d, lab, ms, rounds, change)


_MOVES = ("path_moves", "forest_moves")
_LIST_REFUSALS = ("labels_lists", "upload_primal_lists", "primal_pass_lists")
# defect -> (cell, acts(step): the defect may act at this step, ops that may be the first to show it)
RELABEL_DEFECTS = {
    CostChangeLeavesMovedLabelsOnLists: ("relabel_lists", lambda x: x[0] in ("upload_costs_cold", "upload_costs_warm", "set_constants"), ("ro_labels",)),
    RefusedLabelCallUnsetsLists: ("relabel_lists", lambda x: x[0] == "refused" and x[1][0] in _LIST_REFUSALS, ("ro_labels",)),
    MoveTakesTheLastMinimiser: ("relabel", lambda x: x[0] in _MOVES and x[1][1] > 0, ("labels", "ro_labels")),
    MoveIgnoresOffListNeighbours: ("relabel", lambda x: x[0] in _MOVES and x[1][1] > 0, ("labels", "ro_labels")),
    MoveReadsTheDualsBeforeTheLastPass: ("relabel", lambda x: x[0] in _MOVES and x[1][1] > 0, ("labels", "ro_labels")),
    MoveSkipsThePairwiseSlots: ("relabel", lambda x: x[0] in _MOVES and x[1][1] > 0, ("labels",)),
    StaleMoveSetStillMoves: ("relabel", lambda x: x[0] == "refused" and x[1][0] in ("stale_path_set", "stale_forest_set"), ()),
    UnsetNeighbourCountsAsLabelZero: ("relabel_windows", lambda x: x[0] in _MOVES and x[1][1] > 0, ("labels", "ro_labels")),
}


@pytest.mark.parametrize("defect", list(RELABEL_DEFECTS), ids=lambda d: d.__name__)
def test_a_seeded_defect_of_the_relabelling_calls_fails_a_session_where_it_acts(defect):
    """a committed session of the defect's cell fails: at a step where the defect acts, or at the first observation of the labels
    behind such a step — and never before the first step at which it can act"""
    cell, acts, shows = RELABEL_DEFECTS[defect]
    for seed in SC.CELLS[cell]["seeds"]:
        session = SC.steps(cell, seed)
        try:
            SC.run(defect(), SC.Shadow(), session, observe=None, cell=cell, seed=seed)
        except SC.Mismatch as ex:
            i, msg = ex.index, str(ex)
            break
    else:
        pytest.fail("no committed session of %s notices %s" % (cell, defect.__name__))
    print(defect.__name__, cell, "seed", seed, "noticed at step", i, session[i])
    assert ("session %s seed %d, step %d %s" % (cell, seed, i, session[i][0])) in msg and "the last steps:" in msg
    acting = [k for k in range(i + 1) if acts(session[k])]
    assert acting, (i, session[i])
    if acts(session[i]):
        return
    assert session[i][0] in shows or i == len(session) - 1, (i, session[i])
    if defect in (CostChangeLeavesMovedLabelsOnLists, RefusedLabelCallUnsetsLists):
        # labels that are unset when the step acts show nothing: a move of one round at least came before it
        assert [k for k in range(acting[-1]) if session[k][0] in _MOVES and session[k][1][1] > 0], (acting, i)
