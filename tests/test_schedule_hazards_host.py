"""Every planned schedule against the host-side hazard checker (tests/schedule_hazards.py): footprints pinned against the oracle,
the planner's real Schedule read through tests/cpp/schedule_probe.cpp, every pair of conflicting updates ordered by something the
executor enforces — and proof that the checker reports seeded defects.  No GPU needed."""
import hashlib
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import schedule_hazards as H                     # noqa: E402
import shared_tables_cases as SC                 # noqa: E402
from lp_mp_amd import model as M                 # noqa: E402
from lp_mp_amd import synthetic as S             # noqa: E402
from oracle.binding import Oracle                # noqa: E402

MODES = (M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2, M.REPAM_UNIFORM, M.REPAM_DAMPED_UNIFORM)
MODE_NAMES = ("anisotropic", "anisotropic2", "uniform", "damped_uniform")


@pytest.fixture(scope="module")
def probe_lib(tmp_path_factory):
    return H.build_probe(tmp_path_factory.mktemp("schedule_probe"))


def test_probe_sets_every_chain_setting(probe_lib):
    """the probe hands make_schedule its chain knobs through the environment: one row of its table per member of ChainSettings in
    plan.hpp, in order — a new knob cannot be forgotten silently"""
    fields = H.chain_settings_fields()
    assert len(fields) >= 10
    assert H.probe_setting_names(probe_lib) == fields
    assert sorted(H.SETTING_DEFAULTS) == sorted(fields)


# ---------------------------------------------------------------------------------------------------------------------------
# sweeps

def _sweep(o, d, mode):
    oo, om = o.omega(d, mode)
    mo, mk = o.mask(d, mode)
    return (o.update_order(d), oo, om, mo, mk)


def _plain_sweeps(o, modes=MODES, all_forms=True):
    """(name, segments, fuse) of the directional sweeps and the fused / unfused passes of the weight modes"""
    for mode in modes:
        o.set_reparametrization(mode)
        F, B = _sweep(o, 0, mode), _sweep(o, 1, mode)
        n = MODE_NAMES[mode]
        yield "forward " + n, [F], False
        yield "backward " + n, [B], False
        yield "forward+backward fused " + n, [F, B], True
        yield "backward+forward fused " + n, [B, F], True
        if all_forms:
            yield "forward+backward " + n, [F, B], False
            yield "backward+forward " + n, [B, F], False


def _sublist_sweeps(o, rng, count):
    upd = o.update_order(0)
    for k in range(count):
        keep = rng.uniform(size=len(upd)) < rng.uniform(0.3, 0.9)
        sub = upd[keep] if k % 2 == 0 else upd[keep][::-1].copy()
        if len(sub) == 0:
            continue
        oo, om, mo, mk = o.anisotropic_weights_sublist(sub)
        yield "sub-list %d" % k, [(sub, oo, om, mo, mk)], False


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the footprints are a claim: pin them against the oracle

def _footprint_models():
    """(kind, name, model): the models of the corpus families below, every builder and every kind of message, schedule and flag
    the checker's verdicts rest on; of the two seeded fuzz families the first 8 seeds, of the grid families two label counts in
    both orders (a footprint does not depend on the label count), and not the largest grids (a replay of a 1200-update sweep 20
    times per sweep and mode adds time, no new footprint rule)"""
    for fam in sorted(FAMILIES):
        for k, (name, m, _opt) in enumerate(FAMILIES[fam]()):
            if m.n_factors > 1500 or (fam in ("random_model", "random_bipartite_mrf") and k >= 8) or (fam.endswith(" grids") and k >= 4):
                continue
            yield fam, name, m


def _concat(segs):
    """several (factors, om_off, om, mk_off, mk) as one"""
    f = np.concatenate([s[0] for s in segs])
    om, mk = np.concatenate([s[2] for s in segs]), np.concatenate([s[4] for s in segs])
    oo, mo, a, b = [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], 0, 0
    for s in segs:
        oo.append(np.asarray(s[1][1:], np.int64) + a); mo.append(np.asarray(s[3][1:], np.int64) + b)
        a += int(s[1][-1]); b += int(s[3][-1])
    return f, np.concatenate(oo), om, np.concatenate(mo), mk


def _run(o, d0, rows):
    o.set_duals(d0)
    o.compute_pass_custom(*rows)
    return o.duals()


def test_footprints_are_sufficient_for_the_oracle():
    """conflict-free updates touch disjoint memory: every linear extension of the conflict DAG over the sequential update list — 20
    per sweep, every second one "latest ready first" — gives duals bit-identical to the sequential sweep, for the models of the
    corpus, the directional sweeps and fused passes of all four weight modes and two sub-list passes each.  A footprint that
    forgets an access makes some extension differ.  Conversely the relation is not vacuous: swapping one conflicting adjacent pair
    changes the duals on at least one model of every kind (family)."""
    rng = np.random.default_rng(5)
    swapped, moved, replays = Counter(), Counter(), 0
    for kind, name, m in _footprint_models():
        mi = H.ModelInfo(m)
        o = Oracle(mi.oracle_model)
        d0 = o.duals()
        tried = 0
        for sname, segs, _ in list(_plain_sweeps(o, MODES, all_forms=False)) + list(_sublist_sweeps(o, rng, 2)):
            seq = H.Sequence(mi, *_concat(segs))
            want = _run(o, d0, seq.rows(range(len(seq))))
            edges = seq.edges()
            for k in range(20):
                perm = H.linear_extension(len(seq), edges, rng, adversarial=k % 2 == 1)
                moved[kind] += sum(1 for i, p in enumerate(perm) if i != p)
                assert np.array_equal(_run(o, d0, seq.rows(perm)), want), (name, sname, k)
                replays += 1
            # the converse: conflicting adjacent pairs, swapped (up to three per model)
            for a, b, _v, _kind in edges:
                if b == a + 1 and tried < 3:
                    tried += 1
                    perm = list(range(len(seq)))
                    perm[a], perm[b] = b, a
                    swapped[kind] += not np.array_equal(_run(o, d0, seq.rows(perm)), want)
    print("\nfootprints: %d replays, all equal; swaps that changed the duals per kind: %s" % (replays, dict(swapped)))
    for kind in FAMILIES:
        assert moved[kind] > 0, kind
        assert swapped[kind] > 0, "%s: no swap of a conflicting adjacent pair changes the duals — the relation proves nothing here" % kind


# ---------------------------------------------------------------------------------------------------------------------------
# 4. proof that the checker can fail: seeded defects on the probe's arrays

def _two_forward_sweeps(o):
    o.set_reparametrization(M.REPAM_ANISOTROPIC)
    F = _sweep(o, 0, M.REPAM_ANISOTROPIC)
    return [F, F], False


def _pass(o):
    o.set_reparametrization(M.REPAM_ANISOTROPIC)
    return [_sweep(o, 0, M.REPAM_ANISOTROPIC), _sweep(o, 1, M.REPAM_ANISOTROPIC)], False


def _mutation_models():
    """(name, model, sweep, settings): a deep dense chain with the mailbox (two forward sweeps: every message vector is written
    twice and read twice), the same with completion flags only, a C5-style model in the level loop, and a unary with a `full`
    schedule neighbour under chain_min = 2"""
    grid = S.grid_model(12, 10, 8, order="row_major")
    yield "dense grid, mailbox", grid, _two_forward_sweeps, {}
    yield "dense grid, one sweep", grid, lambda o: (_two_forward_sweeps(o)[0][:1], False), {}
    yield "dense grid, no_mailbox", grid, _two_forward_sweeps, dict(no_mailbox=1)
    yield "dense grid, fused pass", grid, lambda o: (_pass(o)[0], True), {}
    yield "c5 level loop", S.c5_model(8, 8, 4, 200, 120, 40, seed=3, window=16), _pass, {}
    yield "rules_grid full", SC.rules_grid(6, 5, 8, sched=M.SCHED_FULL, seed=8), _pass, dict(chain_min=2)


def _kinds(S_, seq, executor=None):
    v = H.check_all(S_, seq) if executor is None else H.check(S_, seq, executor=executor)
    return Counter(x.kind for x in v), v


def _ordered_pairs(S_, seq):
    """(record a, record b) of the conflicting pairs in different records, with the mapping"""
    rec_of, members = H.map_records(S_, seq, [])
    out = []
    for a, b, _v, _k in seq.edges():
        if rec_of[a] >= 0 and rec_of[b] >= 0 and rec_of[a] != rec_of[b]:
            out.append((rec_of[a], rec_of[b]))
    return rec_of, members, out


def test_checker_flags_every_seeded_defect(probe_lib):
    """every seeded defect is reported, with a violation of the right kind and the two updates named; a defect whose precondition
    a model does not offer is skipped for that model, and each kind fires on at least one model (9, the issue order of the units,
    in the form its comment explains).  The defects are seeded on a copy of the
    arrays the probe returned (H.copy_schedule): the checker reads nothing else."""
    fired = Counter()
    rng = np.random.default_rng(11)
    for name, m, sweep, st in _mutation_models():
        mi = H.ModelInfo(m)
        segs, fuse = sweep(Oracle(mi.oracle_model))
        S0 = H.Probe(probe_lib, m).plan(segs, fuse=fuse, settings=st)
        seq = H.sequence_of(mi, S0)
        assert H.check_all(S0, seq) == [], name
        rec_of, members, pairs = _ordered_pairs(S0, seq)
        launch = S0["rec_launch"]
        # 1. a record of launch k + 1 moved into launch k, next to a record it conflicts with
        for ra, rb in pairs:
            if launch[rb] == launch[ra] + 1:
                T = H.copy_schedule(S0); T["rec_launch"][rb] = launch[ra]
                k, v = _kinds(T, seq, "plain")
                assert k["same_launch"] > 0 and all(x.a is not None and x.b is not None for x in v if x.kind == "same_launch"), (name, 1, v[:2])
                fired[1] += 1
                break
        # 2. two consecutive launches with a conflicting pair, swapped
        for ra, rb in pairs:
            if launch[rb] == launch[ra] + 1:
                T = H.copy_schedule(S0)
                la, lb = launch[ra], launch[rb]
                T["rec_launch"][launch == la] = lb; T["rec_launch"][launch == lb] = la
                k, v = _kinds(T, seq, "plain")
                assert k["launch_order"] > 0, (name, 2, v[:2])
                fired[2] += 1
                break
        for c, ch in enumerate(S0["chains"]):
            n_t = len(ch["tk_launch"])
            if len(ch["dep"]):
                # 3. all dep entries of the chain cleared
                T = H.copy_schedule(S0)
                T["chains"][c]["dep"] = np.zeros(0, np.int64); T["chains"][c]["dep_off"] = np.zeros(n_t + 1, np.int64)
                k, v = _kinds(T, seq, "chain")
                assert k["unordered"] > 0, (name, 3, v[:2])
                fired[3] += 1
                # 4. single dep edges without another path, one at a time
                edges = [(t, j) for t in range(n_t) for j in range(int(ch["dep_off"][t]), int(ch["dep_off"][t + 1]))]
                if len(edges) > 200:
                    edges = [edges[i] for i in rng.choice(len(edges), 200, replace=False)]
                for t, j in edges:
                    d = int(ch["dep"][j])
                    T = H.copy_schedule(S0)
                    T["chains"][c]["dep"] = np.delete(ch["dep"], j)
                    T["chains"][c]["dep_off"] = ch["dep_off"].copy(); T["chains"][c]["dep_off"][t + 1:] -= 1
                    if H.Reach(T["chains"][c]["dep_off"].tolist(), T["chains"][c]["dep"].tolist()).before(("E", d), ("S", t)):
                        continue                                   # another path of flags orders the two tickets
                    k, v = _kinds(T, seq, "chain")
                    assert k["unordered"] > 0, (name, 4, (t, d), v[:2])
                    fired[4] += 1
                # 5. a dep replaced by a higher ticket number
                t = next(t for t in range(n_t) if ch["dep_off"][t + 1] > ch["dep_off"][t])
                if t + 1 < n_t:
                    T = H.copy_schedule(S0); T["chains"][c]["dep"][int(ch["dep_off"][t])] = t + 1
                    k, v = _kinds(T, seq, "chain")
                    assert k["dep_forward"] > 0, (name, 5, v[:2])
                    fired[5] += 1
            if S0["chain_mailbox_rows"][c] > 0:
                lo, hi = int(ch["cl_rec_begin"][0]), int(ch["cl_rec_begin"][-1] + ch["cl_count"][-1])
                ops = [(i, int(S0["rec_op_begin"][i]) + j) for i in range(lo, hi) for j in range(int(S0["rec_n_recv"][i])) if S0["op_mailbox_row"][int(S0["rec_op_begin"][i]) + j] >= 0]
                sends = {int(S0["op_mailbox_row"][int(S0["rec_op_begin"][i] + S0["rec_n_recv"][i]) + j]): (i, int(S0["rec_op_begin"][i] + S0["rec_n_recv"][i]) + j)
                         for i in range(lo, hi) for j in range(int(S0["rec_n_send"][i])) if S0["op_mailbox_row"][int(S0["rec_op_begin"][i] + S0["rec_n_recv"][i]) + j] >= 0}
                vec_of_send = lambda o: (int(S0["op_peer"][o]), int(S0["op_side"][o]))
                i, o = ops[len(ops) // 2]
                row = int(S0["op_mailbox_row"][o])
                # 6. a mailbox receive pointed at another used row
                other = next(r for r in sorted(sends) if vec_of_send(sends[r][1]) != vec_of_send(sends[row][1]))
                T = H.copy_schedule(S0); T["op_mailbox_row"][o] = other
                k, v = _kinds(T, seq, "chain")
                assert k["mailbox_writer"] > 0, (name, 6, v[:2])
                fired[6] += 1
                # 7. ... at the row of an EARLIER writer of the same vector
                for i2, o2 in reversed(ops):
                    r2 = int(S0["op_mailbox_row"][o2])
                    early = [r for r in sorted(sends) if r != r2 and vec_of_send(sends[r][1]) == vec_of_send(sends[r2][1]) and sends[r][0] < sends[r2][0]]
                    if early:
                        T = H.copy_schedule(S0); T["op_mailbox_row"][o2] = early[0]
                        k, v = _kinds(T, seq, "chain")
                        assert k["mailbox_writer"] > 0 and any("last writer" in x.why for x in v), (name, 7, v[:2])
                        fired[7] += 1
                        break
                # 8. the row's send bit deleted: the receive polls a row nobody writes, and nothing else orders the pair
                T = H.copy_schedule(S0); T["op_mailbox_row"][sends[row][1]] = -1
                k, v = _kinds(T, seq, "chain")
                assert k["mailbox_writer"] > 0, (name, 8, v[:2])
                fired[8] += 1
                # ... and OP_MAILBOX cleared on a receive whose pair no path of flags orders: it reads the dual array too early
                ex = H.Executor(S0, "chain", [])
                flags = H.Reach(ch["dep_off"].tolist(), ch["dep"].tolist())
                for i2, o2 in ops:
                    w = sends[int(S0["op_mailbox_row"][o2])][0]
                    if not flags.before(("E", ex.ticket[w]), ("S", ex.ticket[i2])):
                        T = H.copy_schedule(S0); T["op_mailbox_row"][o2] = -1
                        k, v = _kinds(T, seq, "chain")
                        assert k["unordered"] > 0, (name, "8b", v[:2])
                        fired["8b"] += 1
                        break
        # 9. the issue order of the units, first form: the LAST launch of a level loop taken out of its chain and issued as a plain
        # launch, i.e. before the chain that feeds it (Schedule::chains reordered: after this loop)
        assert H.check(S0, seq, executor="chain").stats["cross_unit_pairs"] == 0, name
        for c, ch in enumerate(S0["chains"]):
            if S0["chain_level_loop"][c] and len(ch["cl_count"]) >= 2:
                last = int(np.flatnonzero(S0["launch_begin"] == ch["cl_rec_begin"][-1])[0])
                if not any(launch[rb] == last and launch[ra] != last for ra, rb in pairs):
                    continue
                T = H.copy_schedule(S0)
                for key in ("cl_rec_begin", "cl_count", "cl_ticket0", "cl_flags"):
                    T["chains"][c][key] = ch[key][:-1].copy()
                T["plain_launches"] = np.concatenate([S0["plain_launches"], [last]])
                k, v = _kinds(T, seq, "chain")
                assert k["unordered"] > 0 and any("issue order" in x.why for x in v), (name, 9, v[:2])
                fired[9] += 1
        # 10. one send op dropped from a record
        i = next(i for i in range(len(launch)) if S0["rec_n_send"][i] > 0)
        T = H.copy_schedule(S0); T["rec_n_send"][i] -= 1
        k, v = _kinds(T, seq, "plain")
        assert k["mapping"] > 0, (name, 10, v[:2])
        fired[10] += 1
        # 11. two updates of one factor folded into one record across an update that conflicts with the second
        for ra, rb in pairs:
            f = int(S0["rec_factor"][rb])
            mine = [i for i in range(len(launch)) if S0["rec_factor"][i] == f and i != rb and members[i] and members[i][0] < members[ra][0] and len(members[i]) == 1 and len(members[rb]) == 1]
            if not mine or members[ra][0] > members[rb][0]:
                continue
            i1 = max(mine, key=lambda i: members[i][0])
            if any(members[i1][0] < members[x][0] < members[rb][0] for x in range(len(launch)) if S0["rec_factor"][x] == f and x not in (i1, rb) and members[x]):
                continue
            T = H.copy_schedule(S0)
            r1, s1 = _ops_of(S0, i1)
            r2, s2 = _ops_of(S0, rb)
            new = r1 + r2 + s1 + s2
            for key in H._OP:
                T[key] = np.concatenate([S0[key], S0[key][new]])
            T["rec_op_begin"][i1] = len(S0["op_peer"]); T["rec_n_recv"][i1] = len(r1) + len(r2); T["rec_n_send"][i1] = len(s1) + len(s2)
            for key in H._REC:
                T[key] = np.delete(T[key], rb)
            k, v = _kinds(T, seq, "plain")
            assert k["fold"] > 0 and k["mapping"] == 0, (name, 11, v[:2])
            fired[11] += 1
            break
    # 9 as stated: Schedule::chains reordered on a model with a conflicting pair in two chains.  The planner refuses to chain a
    # schedule with a dependency between classes it sees; the one it does not see is between two pairwise factors that round
    # themselves and share a unary (their touch of the unaries' labels in a primal pass), in different classes.  engine.cpp never
    # runs that pass in the chain form, so the pair needs no order there — with primal_in_chain the checker is told to demand one,
    # and only the issue order of the two chains gives it
    from test_fuzz_gpu import random_mrf_rounding_pairwise
    m = random_mrf_rounding_pairwise(np.random.default_rng(17007))
    mi = H.ModelInfo(m)
    o = Oracle(m)
    probe = H.Probe(probe_lib, m, force_generic=True)
    for sname, segs, fuse in list(_plain_sweeps(o)) + list(_sublist_sweeps(o, np.random.default_rng(9), 24)):
        S0 = probe.plan(segs, fuse=fuse, settings=dict(chain_min=2))
        seq = H.sequence_of(mi, S0)
        r = H.check(S0, seq, executor="chain", primal_in_chain=True)
        if len(S0["chains"]) < 2 or r.stats["cross_unit_pairs"] == 0:
            continue
        assert r == [] and H.check_all(S0, seq) == [], sname
        T = H.copy_schedule(S0)
        T["chains"] = T["chains"][::-1]
        for key in ("chain_class", "chain_block_records", "chain_level_loop", "chain_banded", "chain_valid", "chain_mailbox_rows", "chain_mailbox_width"):
            T[key] = T[key][::-1].copy()
        v = H.check(T, seq, executor="chain", primal_in_chain=True)
        assert any(x.kind == "unordered" and "issue order" in x.why for x in v), (sname, v[:2])
        fired["9 chains reordered"] += 1
        break
    print("\nseeded defects reported:", dict(sorted(fired.items(), key=str)))
    assert [k for k in list(range(1, 12)) + ["8b", "9 chains reordered"] if fired[k] == 0] == [], fired


def _ops_of(S_, i):
    ob, nr, ns = int(S_["rec_op_begin"][i]), int(S_["rec_n_recv"][i]), int(S_["rec_n_send"][i])
    return list(range(ob, ob + nr)), list(range(ob + nr, ob + nr + ns))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the corpus

BAND = dict(band_min_set=1, band_min_bytes=1, band_bytes=64)
SETTINGS = [
    ("default", {}, {}),
    ("chain_min=2", dict(chain_min=2), {}),
    ("chain_all", dict(chain_min=2, chain_all=1), {}),
    ("no_mailbox", dict(chain_min=2, no_mailbox=1), {}),
    ("no_level_loop", dict(chain_min=2, no_level_loop=1), {}),
    ("budget 0", dict(chain_min=2), dict(mailbox_budget_bytes=0)),
    ("budget partial", dict(chain_min=2), dict(mailbox_budget_bytes="partial")),
    ("banded", dict(BAND), {}),
    ("banded chain_min=2", dict(BAND, chain_min=2), {}),
    ("no_blocked_passes", dict(BAND, no_blocked_passes=1), {}),
    ("heavy", dict(chain_min=2, heavy_bytes=1), {}),
    ("force_generic", dict(chain_min=2), dict(force_generic=True)),
]
COVERAGE = Counter()
FAMILIES_RUN = set()
DENSE_EXACT = range(1, 5)


def _count(S_, settings, kw, report, default_S):
    c = COVERAGE
    members = report.members
    chains = S_["chains"]
    n_launches = len(S_["launch_class"])
    c["schedules"] += 1
    if not chains:
        c["plain schedules"] += 1
    for k, ch in enumerate(chains):
        if S_["chain_level_loop"][k]:
            c["level loops"] += 1
            c["LABEL_OPS launches"] += int(np.sum((ch["cl_flags"] & H.CHAIN_LAUNCH_LABEL_OPS) != 0))
            c["LABEL_PAIRED launches"] += int(np.sum((ch["cl_flags"] & H.CHAIN_LAUNCH_LABEL_PAIRED) != 0))
        elif S_["chain_mailbox_rows"][k] > 0:
            c["mailbox chains"] += 1
        else:
            c["flag chains"] += 1
            c["flag chains with dependencies"] += len(ch["dep"]) > 0
        if S_["chain_banded"][k]:
            c["banded chains"] += 1
    c["folded records"] += sum(1 for m in members if len(m) > 1)
    c["records in indirect launches"] += int(sum(S_["launch_end"][li] - S_["launch_begin"][li] for li in range(n_launches) if S_["launch_stride"][li] < 0))
    split = Counter((int(S_["launch_level"][li]), int(S_["launch_class"][li])) for li in range(n_launches) if H.kc_is_shared(int(S_["launch_class"][li])))
    c["shared-class launches split by table set"] += sum(n - 1 for n in split.values() if n > 1)
    early_exit = not chains and len(S_["plain_launches"]) == 0 and n_launches >= settings.get("chain_min", 9)
    capable = all(H.kc_is_packed(int(k)) or int(k) in (H.KC_GENERIC, H.KC_SMALL) for k in S_["launch_class"])
    # replay refused (a dependency between two kernel classes): nothing else ends chain planning without a chain and without a
    # plain launch when every class alone is long enough, all are chain-capable, the launches are not heavy — and the checker's own
    # pairs hold one between two classes
    per_class = Counter(S_["launch_class"].tolist())
    if early_exit and capable and "heavy_bytes" not in settings and len(per_class) > 1 and min(per_class.values()) >= settings.get("chain_min", 9) \
            and report.stats["cross_class_pairs"] > 0:
        c["cross-class exits"] += 1
    if default_S is not None:
        had = len(default_S["chains"]) > 0
        if "heavy_bytes" in settings and had and early_exit:
            c["heavy exits"] += 1
        if "mailbox_budget_bytes" in kw and int(np.sum(default_S["chain_mailbox_rows"])) > int(np.sum(S_["chain_mailbox_rows"])):
            c["chains where the budget dropped the mailbox"] += 1
            if int(np.sum(S_["chain_mailbox_rows"])) > 0:
                c["budgets that admit some classes only"] += 1
    # the banded order was tried (chain planning reached its per-class loop: there are chains or plain launches) and no lag kept
    # the dependencies backwards
    if settings.get("band_min_set") and not settings.get("no_blocked_passes") and (chains or len(S_["plain_launches"])):
        for cls in DENSE_EXACT:
            steps = [li for li in range(n_launches) if S_["launch_class"][li] == cls]
            tables = [li for li in steps if S_["launch_n_recv"][li] > 0]
            if 2 <= len(steps) <= 8 and len(tables) >= 2 and not any(S_["chain_banded"][k] and S_["chain_class"][k] == cls for k in range(len(chains))):
                c["banded refused"] += 1


def _digest(S_):
    h = hashlib.sha1()
    for k in sorted(S_):
        if isinstance(S_[k], np.ndarray):
            h.update(k.encode()); h.update(S_[k].tobytes())
    for ch in S_["chains"]:
        for k in sorted(ch):
            h.update(k.encode()); h.update(ch[k].tobytes())
    return h.digest()


def _check_model(L, name, m, sweeps_of, settings=SETTINGS, failures=None, partition=False, rng=None):
    mi = H.ModelInfo(m)
    probes = {}

    def probe(**kw):
        key = tuple(sorted(kw.items()))
        if key not in probes:
            probes[key] = H.Probe(L, m, **kw)
        return probes[key]
    o = Oracle(mi.oracle_model)
    jobs = [(sname, dict(segments=segs, fuse=fuse)) for sname, segs, fuse in sweeps_of(o)]
    if partition:
        for rtype in (2, 3):
            for inner in (1, 5):
                jobs.append(("partition pass rtype %d inner %d" % (rtype, inner), dict(partition=(rtype, inner))))
    rounds_pairwise = any(mi.primal_type[f] and mi.pairwise[f] for f in range(mi.nf))
    for sname, how in jobs:
        seq, verdicts = None, {}
        default_S = None
        for stname, st, kw in settings:
            kw = dict(kw)
            if kw.get("mailbox_budget_bytes") == "partial":
                base = probe().plan(settings=st, **how)
                sizes = sorted(int(r) * int(w) * 16 for r, w in zip(base["chain_mailbox_rows"], base["chain_mailbox_width"]) if r > 0)
                if len(sizes) < 2:
                    continue
                kw["mailbox_budget_bytes"] = sizes[0]
            S_ = probe(**kw).plan(settings=st, **how)
            if seq is None:
                seq = H.sequence_of(mi, S_)
                if "partition" in how:
                    COVERAGE["partition segments"] += len(S_["seg_n"])
            if stname == "default":
                default_S = S_
            base_S = default_S
            if "heavy_bytes" in st or "mailbox_budget_bytes" in kw:
                base_S = probe().plan(settings={k2: v for k2, v in st.items() if k2 != "heavy_bytes"}, **how)
            # (settings that do not bear on a sweep give the same schedule byte for byte: the same verdict, not computed again)
            key = _digest(S_)
            if key not in verdicts:
                v = H.check_all(S_, seq)
                if rounds_pairwise and len(S_["chains"]):
                    # engine.cpp never runs a primal pass of such a model in the chain form; if it did, the rule "a pairwise factor
                    # that rounds itself touches all its unaries" would have to be ordered there too — by the issue order of the
                    # units, since chain_plan.cpp replay does not visit those accesses.  Checked as well, and counted: the model of
                    # seeded defect 9
                    w = H.check(S_, seq, executor="chain", primal_in_chain=True)
                    v.stats["cross_unit_pairs_primal"] = w.stats["cross_unit_pairs"]
                    v += [x for x in w if repr(x) not in {repr(y) for y in v}]
                verdicts[key] = v
            else:
                COVERAGE["schedules equal to one already checked"] += 1
            v = verdicts[key]
            COVERAGE["pairs between two units if primal passes ran in the chain form"] += v.stats["cross_unit_pairs_primal"]
            COVERAGE["conflicting pairs checked"] += v.stats["pairs"]
            COVERAGE["pairs ordered by a mailbox row itself"] += v.stats["pairs_ordered_by_the_row_itself"]
            COVERAGE["pairs between two units of a chained schedule"] += v.stats["cross_unit_pairs"]
            if v:
                failures.append("%s | %s | %s: %d violations, first %r" % (name, sname, stname, len(v), v[:2]))
                continue
            _count(S_, st, kw, v, base_S)


def _fam_builders():
    from test_plan_host import _toy, _full_schedule_model, _hub_model, _duplicate_message_model
    yield "toy", _toy(), {}
    yield "every schedule", _full_schedule_model(), {}
    for pw in ("dense", "potts"):
        yield "hub 16 x 40 " + pw, _hub_model(16, 40, pw), dict(modes=(M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM))
    yield "hub 8 x 12", _hub_model(8, 12, "dense"), {}
    for Lb in (4, 5, 16):
        yield "duplicate messages %d" % Lb, _duplicate_message_model(Lb), {}
    yield "chain", S.chain_model(40, 4), {}


def _fam_grids(pairwise):
    def gen():
        for Lb in (3, 4, 7, 8, 16, 32, 40):
            for order in ("row_major", "colour_major"):
                kw = dict(n_tables=3) if pairwise == "shared" else {}
                yield "%s grid 6x5 L%d %s" % (pairwise, Lb, order), S.grid_model(6, 5, Lb, pairwise=pairwise, order=order, seed=Lb, **kw), \
                    dict(modes=MODES if Lb in (4, 7) else (M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM))
    return gen


def _two_component_model(n=14):
    """two paths of variables with 4 and 8 labels in ONE model: two packed classes, each deep enough for a chain with a mailbox
    and no dependency between them — the shape in which a mailbox budget can admit one class and not the other"""
    mt = [M.MsgType(0, 1, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(0, 1, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1),
          M.MsgType(2, 3, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(2, 3, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1)]
    b = M.ModelBuilder(4, mt)
    rng = np.random.default_rng(3)
    for k, Lb in enumerate((4, 8)):
        u = b.add_vector_factors(2 * k, rng.uniform(0, 1, (n, Lb)))
        p = b.add_dense_pairwise(2 * k + 1, rng.uniform(0, 1, (n - 1, Lb, Lb)))
        for i in range(n - 1):
            b.add_messages(2 * k, u[i], p[i]); b.add_messages(2 * k + 1, u[i + 1], p[i])
            b.add_relations([u[i], p[i]], [p[i], u[i + 1]])
    return b.finish()


def _crossed_bipartite_model(n=320, Lb=32):
    """two sides of n variables in colour-major order, variable i of side A joined to variables i and n - 1 - i of side B: the first
    block of B's step waits for the LAST block of A's step, so no lag of the skewed band order keeps every dependency backwards and
    the banded order is refused (72 blocks of four records per step: more than 17 bands)"""
    i = np.arange(n)
    ei = np.concatenate([i, i])
    ej = np.concatenate([n + i, n + (n - 1 - i)])
    keep = np.unique(np.stack([ei, ej], 1), axis=0)
    return S.mrf_model(2 * n, Lb, keep[:, 0], keep[:, 1], S.u01(2 * n * Lb, 3), tables=S.u01(len(keep) * Lb * Lb, 4))


def _fam_deep():
    yield "crossed bipartite 320 + 320, 32 labels", _crossed_bipartite_model(), dict(modes=(M.REPAM_ANISOTROPIC,), sublists=0)
    yield "two components, 4 and 8 labels", _two_component_model(), dict(modes=(M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM))
    yield "dense grid 40x30 L8 row_major", S.grid_model(40, 30, 8, order="row_major"), dict(modes=(M.REPAM_ANISOTROPIC,))
    yield "potts grid 24x20 L7 row_major", S.grid_model(24, 20, 7, pairwise="potts", order="row_major"), dict(modes=(M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM))
    yield "shared grid 13x11 L32 row_major", S.grid_model(13, 11, 32, pairwise="shared", order="row_major", n_tables=2), dict(modes=(M.REPAM_ANISOTROPIC,))
    yield "shared grid 12x9 L8 11 tables", SC.budget_grid(12, 9, 8, "row_major", 11), dict(modes=(M.REPAM_ANISOTROPIC,))
    yield "shared grid 20x20 L32 40 tables", SC.budget_grid(20, 20, 32, "colour_major", 40), dict(modes=(M.REPAM_ANISOTROPIC,))
    yield "c5 24x24 window 16", S.c5_model(24, 24, 8, 400, 300, 100, seed=5, window=16), dict(modes=(M.REPAM_ANISOTROPIC,))


def _fam_structured():
    yield "counter graph", S.counter_graph_model(60, 150, 4, 3), {}
    yield "counter graph 16 labels", S.counter_graph_model(80, 400, 16, 2), dict(modes=(M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM))
    yield "c5 window 16", S.c5_model(8, 8, 4, 200, 120, 40, seed=3, window=16), {}
    yield "c5 global triples", S.c5_model(8, 8, 4, 200, 120, 40, seed=3, window=200), dict(modes=(M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM))
    yield "c5 no higher-order factors", S.c5_model(6, 6, 8, 30, 0, 0, seed=2), dict(modes=(M.REPAM_ANISOTROPIC,))
    yield "c5 coloured edge variables", S.c5_model(6, 7, 8, 120, 90, 30, seed=4, window=16, colour_edge_vars=True), dict(modes=(M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM))
    yield "multicut", S.multicut_triangle_model(12, 15, seed=4), {}
    yield "multicut 30", S.multicut_triangle_model(30, 40, seed=5), dict(modes=(M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM))
    yield "random graph potts 16", S.random_graph_model(60, 200, 16, seed=4, pairwise="potts"), dict(modes=(M.REPAM_ANISOTROPIC,))


N_FUZZ = 60


def _fam_fuzz_random():
    from test_fuzz_gpu import random_model, random_rows
    for seed in range(N_FUZZ):
        rng = np.random.default_rng(1000 + seed)
        m = random_model(rng)
        yield "random_model %d" % seed, m, dict(modes=(MODES[seed % 4],), all_forms=seed % 2 == 0, sublists=1, random_rows=(random_rows, rng))


def _fam_fuzz_bipartite():
    from test_fuzz_gpu import random_bipartite_mrf
    for seed in range(N_FUZZ):
        m = random_bipartite_mrf(np.random.default_rng(17000 + seed))
        yield "random_bipartite_mrf %d" % seed, m, dict(modes=(MODES[seed % 4],), all_forms=seed % 2 == 0, sublists=1)


def _fam_shared_cases():
    for seed in range(6):
        yield "mixed_graph %d" % seed, SC.mixed_case(seed), dict(modes=(MODES[seed % 4], M.REPAM_ANISOTROPIC))
    for seed in range(8):
        yield "mixed fuzz %d" % seed, SC.fuzz_case(seed)[0], dict(modes=(MODES[seed % 4],))
    for sched in (M.SCHED_LEFT, M.SCHED_RIGHT, M.SCHED_FULL):
        for Lb in (3, 8):
            yield "rules_grid schedule %d L%d" % (sched, Lb), SC.rules_grid(6, 5, Lb, sched=sched, seed=Lb), dict(modes=(M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM))
    yield "rules_grid blocks", SC.rules_grid(6, 7, 8, order="colour_major", seed=3, blocks=3), dict(modes=(M.REPAM_ANISOTROPIC,), partition=True)
    yield "rules_grid blocks row-major full", SC.rules_grid(6, 7, 4, order="row_major", seed=5, blocks=2, sched=M.SCHED_FULL), dict(modes=(M.REPAM_ANISOTROPIC,), partition=True)
    yield "rules_grid batch sends", SC.rules_grid(5, 6, 4, seed=2, sched=M.SCHED_FULL, flags=M.MF_BATCH_TO_RIGHT | M.MF_BATCH_TO_LEFT), dict(modes=(M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM))
    yield "rect chain", SC.rect_chain(), dict(modes=(M.REPAM_ANISOTROPIC,))
    yield "rect chain 3 x 27", SC.rect_chain(n=12, seed=8, dims=(3, 27)), dict(modes=(M.REPAM_ANISOTROPIC,))


def _fam_primal():
    from test_fuzz_gpu import random_mrf_rounding_pairwise
    for seed in range(12):
        yield "pairwise factors round themselves %d" % seed, random_mrf_rounding_pairwise(np.random.default_rng(17000 + seed)), dict(modes=(MODES[seed % 4],))
    yield "grid compute_primal", S.grid_model(6, 5, 8, order="row_major", seed=7, compute_primal=True), dict(modes=(M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM))
    yield "shared grid compute_primal", SC.primal_grid(5, "colour_major"), dict(modes=(M.REPAM_ANISOTROPIC,))
    yield "dense grid blocks", _partition_grid(), dict(modes=(M.REPAM_ANISOTROPIC,), partition=True)


def _partition_grid():
    """a dense row-major grid with put_in_same_partition blocks of three columns (the model of
    test_oracle_partition_and_adaptive_rules_are_dual_ascent)"""
    Hh, W, Lb = 5, 6, 4
    a, bb = S.grid_edges(Hh, W)
    b = M.ModelBuilder(2, S.mrf_mtypes())
    u = b.add_vector_factors(0, S.u01(Hh * W * Lb, 7).reshape(-1, Lb))
    p = b.add_dense_pairwise(1, S.u01(len(a) * Lb * Lb, 8).reshape(-1, Lb, Lb))
    b.add_interleaved_messages(np.tile(np.array([0, 1], np.int32), len(a)), np.stack([u[a], u[bb]], 1).reshape(-1), np.repeat(p, 2))
    b.add_relations(np.stack([u[a], p], 1).reshape(-1), np.stack([p, u[bb]], 1).reshape(-1))
    for k in range(len(a)):
        if (a[k] % W) // 3 == (bb[k] % W) // 3:
            b.put_in_same_partition(u[a[k]], u[bb[k]])
    return b.finish()


def _fam_labeling_shapes():
    """labeling-list models whose left factor has several labelings (tests/labeling_cases.py): one case per family, shape and
    message schedule (the implicit-origin flags do not bear on a schedule)"""
    import labeling_cases as LC
    for c in LC.CASES.values():
        if c.io == c.fam.io:
            yield c.name, LC.build(c), dict(modes=(M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM), all_forms=c.shape != "chain" or c.sched != "left", sublists=1)


FAMILIES = {
    "labeling shapes": _fam_labeling_shapes,
    "builders of test_plan_host": _fam_builders,
    "dense grids": _fam_grids("dense"),
    "potts grids": _fam_grids("potts"),
    "shared grids": _fam_grids("shared"),
    "deep schedules": _fam_deep,
    "structured models": _fam_structured,
    "random_model": _fam_fuzz_random,
    "random_bipartite_mrf": _fam_fuzz_bipartite,
    "shared-table cases": _fam_shared_cases,
    "rounding and partitions": _fam_primal,
}


def _run_family(L, fam):
    failures = []
    rng = np.random.default_rng(len(fam))
    for name, m, opt in FAMILIES[fam]():
        def sweeps_of(o, opt=opt):
            yield from _plain_sweeps(o, opt.get("modes", MODES), opt.get("all_forms", True))
            yield from _sublist_sweeps(o, rng, opt.get("sublists", 2))
            if "random_rows" in opt:
                fn, r = opt["random_rows"]
                for k in range(2):
                    yield "random rows %d" % k, [fn(r, None, o, m)], False
        _check_model(L, name, m, sweeps_of, failures=failures, partition=opt.get("partition", False))
    FAMILIES_RUN.add(fam)
    return failures


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_planned_schedule_is_hazard_free(probe_lib, family):
    """every schedule the planner emits for the corpus — directional sweeps, fused and unfused passes of all four weight modes,
    sub-list passes, random rows, partition passes — under every chain setting: each pair of conflicting updates is ordered by
    launch order, issue order, dep edges or a mailbox hand-over, in both execution forms.  A failure names model | sweep | setting."""
    failures = _run_family(probe_lib, family)
    assert not failures, "\n".join(failures[:20])


REQUIRED = ("plain schedules", "flag chains", "flag chains with dependencies", "mailbox chains", "chains where the budget dropped the mailbox",
            "budgets that admit some classes only",
            "banded chains", "banded refused", "level loops", "LABEL_OPS launches", "LABEL_PAIRED launches", "folded records", "cross-class exits",
            "heavy exits", "shared-class launches split by table set", "records in indirect launches", "partition segments",
            "pairs ordered by a mailbox row itself", "pairs between two units if primal passes ran in the chain form")


def test_the_corpus_reached_every_branch_of_the_planner(probe_lib):
    """the coverage counters accumulated by test_every_planned_schedule_is_hazard_free (families not run yet in this session are
    run here): every branch of chain planning was reached by a schedule that was then checked"""
    for fam in sorted(FAMILIES):
        if fam not in FAMILIES_RUN:
            assert not _run_family(probe_lib, fam), fam
    print("\nschedule hazard corpus coverage:")
    for k in sorted(COVERAGE):
        print("  %-50s %d" % (k, COVERAGE[k]))
    missing = [k for k in REQUIRED if COVERAGE[k] <= 0]
    assert not missing, missing
    # the planner never chains a schedule with a dependency between kernel classes (chain_plan.cpp replay): no pair of conflicting
    # updates lies in two different units of a chained schedule, which is why reordering Schedule::chains cannot be seeded as a defect
    assert COVERAGE["pairs between two units of a chained schedule"] == 0
