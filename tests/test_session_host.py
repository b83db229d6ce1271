"""The session tests without a GPU (tests/session_cases.py): the generator is deterministic and covers what it claims, the harness
runs end to end with a second shadow in the engine's place and agrees with a straight replay through the plain oracle, and it notices
the defects it is for — engines with one seeded defect each make a session fail at the defective call or the first observation
after it.  A green run of tests/test_session_gpu.py means what these tests make it mean."""
import collections
import dataclasses

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
        assert len(ups) == 4 and all(15 <= b - a - 4 <= 36 for a, b in zip(ups, ups[1:]))
        rtype = 0
        for i, (op, a) in enumerate(s):                 # the send rule stays across uploads: SHARED when a model comes that draws no other
            rtype = a[0] if op == "set_reparametrization_type" else rtype
            assert not (op == "upload" and not SC.props(a[0])["mrf"] and rtype != 0), (seed, i)
        for i in ups[1:]:
            assert s[i + 1] == ("refused", ("stale_readout", s[i + 1][1][1])) and s[i + 2][:1] == ("refused",) and s[i + 2][1][0] == "stale_schedule"


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
    rtype, slots = 0, {}

    def rebuild(duals):
        m = RP.with_duals(raw, duals)
        q = Oracle(MP.oracle_model(m) if prec != "f64" else RC.oracle_model(m))
        q.set_reparametrization_type(rtype)
        if mode is not None:
            q.set_reparametrization(mode)
        return q

    for i, (op, a) in enumerate(session):
        if op == "upload":
            key, prec, mode, slots = a[0], a[2], None, {}
            raw = SC.model_with_costs(key, a[1], prec == "f32")
            nominal = raw.dual_data
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
            f = RP.listed_subset(raw, a[0])
            raw = RP.with_rows(raw, f, RP.rows_for(raw, f, a[0], float_valued=prec == "f32"))
            o = rebuild(o.duals())
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


@pytest.mark.parametrize("cell", ["diffpool", "mixed4", "deep", "hop"])
def test_replay_with_a_fresh_engine_in_the_middle(cell):
    """tests/session_replay.py --fresh-at K: a new engine takes over with the shadow's model, duals, mode, read-outs, schedules and
    labels — K right behind a step that sets labels which a later step still observes (no cost change in between unsets them)"""
    unsets = ("upload", "upload_costs_cold", "upload_costs_warm", "set_constants", "upload_shared_pool")
    k = None
    for seed in (SC.HOP_SEEDS if cell == "hop" else SC.CELLS[cell]["seeds"]):
        s = SC.steps(cell, seed)
        for i in [i for i, (op, a) in enumerate(s) if op == "decode_primal" or op.endswith("_and_primal")]:
            j = next((j for j in range(i + 1, len(s)) if s[j][0] in ("labels", "ro_labels") or s[j][0] in unsets), None)
            if j is not None and s[j][0] not in unsets:
                k = i + 1
                break
        if k is not None:
            break
    assert k is not None
    SC.run([SC.Shadow()], SC.Shadow(), s, observe=None, cell=cell, seed=seed, fresh_at=k, fresh=SC.Shadow)
