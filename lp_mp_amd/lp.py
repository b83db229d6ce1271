"""Host-side mirror of the reference's plug-in surface for the sweep path, in Python.

Same names, argument meaning and error behaviour as the reference (paths relative to /root/reference):

  FMC / FactorContainer / MessageContainer   test/test_model.hxx:130-137, include/factors_messages.hxx:571-578
  LP<FMC>                                     include/LP_MP.h:239-285 (add_factor/add_message), :698-728, :330,
                                              :869-911 (ComputePass...), :981-1005 (iterator-range ComputePass),
                                              :412-460 (get_omega), :1507-1518 (LowerBound), :462 (add_to_constant)
  Solver::Solve                               include/solver.hxx:230-287
  StandardVisitor                             include/visitors/standard_visitor.hxx:28-199
  LpControl / LPReparametrizationMode         include/config.hxx:71-105

The factor and message OPS that can be plugged in are the device-capable kinds: a user op that is not
one of them is rejected when the FMC is declared (there is no CPU fallback that would silently run it).
The compute itself happens in the HIP engine behind the C ABI (include/lpmp_engine.h).
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import model as M
from .engine import Engine, EngineError


# ---- factor ops (what the reference calls FACTOR_TYPE) -------------------------------------------------
class UnarySimplexFactor:
    """cost vector over the labels of one variable (reference test/simplex.cpp:8-12)."""
    kind = M.F_VECTOR
    implicit_origin = False

    def __init__(self, cost: Sequence[float]):
        self.cost = np.asarray(cost, np.float64).reshape(-1)


class ConstantFactor(UnarySimplexFactor):
    """factor without variables that carries an offset (reference include/factors/constant_factor.hxx:10-30): dual =
    the offset, LowerBound = the offset; on the device a vector factor with one entry."""

    def __init__(self, offset: float = 0.0):
        super().__init__([offset])

    def AddToOffset(self, delta: float):
        self.cost[0] += delta


class test_factor(UnarySimplexFactor):
    """two-label toy factor (reference test/test_model.hxx:10-64)."""

    def __init__(self, x: float, y: float):
        super().__init__([x, y])


class PairwiseSimplexFactor:
    """dense table + one message vector per side (reference test/simplex.cpp:52-65)."""
    kind = M.F_PAIRWISE_DENSE

    def __init__(self, dim1: int, dim2: int, cost=None):
        self.dim1, self.dim2 = int(dim1), int(dim2)
        self.table = np.zeros((dim1, dim2)) if cost is None else np.asarray(cost, np.float64).reshape(dim1, dim2)

    def cost(self, x1, x2):
        return self.table[x1, x2]


class pairwise_potts_factor:
    """diff * [x1 != x2] (reference test/potts_factor.cpp:34-36)."""
    kind = M.F_PAIRWISE_POTTS

    def __init__(self, dim: int, diff_cost: float):
        self.dim, self.diff = int(dim), float(diff_cost)


class shared_pairwise_factor:
    """scale * V[x1][x2] with V a table of the LP's pool (LP.add_shared_table): the engine's F_PAIRWISE_SHARED kind — one double
    per factor, the table read from on-chip memory by the sweep.  Usable in a FactorContainer wherever PairwiseSimplexFactor is
    (the same UnaryPairwiseMessage ops): ``lp.add_factor(P, table_id, scale)``."""
    kind = M.F_PAIRWISE_SHARED

    def __init__(self, table_id: int, scale: float = 1.0):
        self.table_id, self.scale = int(table_id), float(scale)
        self.table = None                   # bound by LP.add_factor

    @property
    def dim1(self) -> int:
        return int(self.table.shape[0])

    @property
    def dim2(self) -> int:
        return int(self.table.shape[1])

    def cost(self, x1, x2):
        return np.float64(self.scale) * self.table[x1, x2]


class diff_pairwise_factor:
    """scale * D[x1 - x2 + dim2 - 1] with D a vector of the LP's pool (LP.add_diff_table): the engine's F_PAIRWISE_DIFF kind — one
    double per factor, no table in memory.  ``lp.add_factor(P, table_id, dim1, dim2, scale)`` in a container of its own; an
    instance may also be handed to a container of PairwiseSimplexFactor or shared_pairwise_factor (the same
    UnaryPairwiseMessage ops, the same dual layout): ``lp.add_factor(P, diff_pairwise_factor(...))``."""
    kind = M.F_PAIRWISE_DIFF

    def __init__(self, table_id: int, dim1: int, dim2: int, scale: float = 1.0):
        self.table_id, self.dim1, self.dim2, self.scale = int(table_id), int(dim1), int(dim2), float(scale)
        self.vec = None                     # bound by LP.add_factor

    def cost(self, x1, x2):
        return np.float64(self.scale) * self.vec[np.asarray(x1) - np.asarray(x2) + self.dim2 - 1]


class diff_shift_pairwise_factor:
    """scale * D[clip(x1 - x2 + shift, 0, n - 1)] with D a vector of ANY length n of the LP's pool (LP.add_diff_table): the engine's
    F_PAIRWISE_DIFF_SHIFT kind — two doubles per factor {scale, shift}, no table in memory.  The clamped index continues D with its
    end values; ``shift`` is an integer with |shift| <= 2^30 (model.window_shift gives the one of two label windows).
    ``lp.add_factor(P, dim1, dim2, table_id, scale, shift)`` in a container of its own; a ready instance is interchangeable in a
    tabled container as a diff_pairwise_factor is.  ``set_factor_cost`` replaces scale and shift (not the vector or the dims)."""
    kind = M.F_PAIRWISE_DIFF_SHIFT

    def __init__(self, dim1: int, dim2: int, table_id: int, scale: float = 1.0, shift: int = 0):
        self.table_id, self.dim1, self.dim2, self.scale = int(table_id), int(dim1), int(dim2), float(scale)
        try:
            self.shift = int(M.check_diff_shifts(shift, "diff_shift_pairwise_factor")[0])
        except ValueError as e:
            raise RuntimeError(str(e)) from None
        self.vec = None                     # bound by LP.add_factor

    def cost(self, x1, x2):
        return np.float64(self.scale) * self.vec[np.clip(np.asarray(x1) - np.asarray(x2) + self.shift, 0, self.vec.shape[0] - 1)]


def labeling_factor(labelings: Sequence[Sequence[int]], implicit_origin: bool):
    """labeling_factor<labelings<...>, IMPLICIT_ORIGIN> (reference include/factors/labeling_list_factor.hxx:220)."""
    labs = [tuple(l) for l in labelings]

    class _LabelingFactor:
        kind = M.F_VECTOR
        labelings = labs

        def __init__(self, cost=None):
            self.cost = np.zeros(len(labs)) if cost is None else np.asarray(cost, np.float64).reshape(len(labs))

    _LabelingFactor.implicit_origin = bool(implicit_origin)
    return _LabelingFactor


# ---- message ops (MESSAGE_TYPE) ------------------------------------------------------------------------
@dataclass(frozen=True)
class UnaryPairwiseMessage:
    """UnaryPairwiseMessage<Chirality> (reference test/simplex_marginalization.cpp:19-20); side 0 = left variable."""
    side: int
    kind: int = M.M_UNARY_PAIRWISE
    flags: int = 0      # M.MF_*: optional members of the op (improvement for adaptive sends, static batch sends)


@dataclass(frozen=True)
class labeling_message:
    """labeling_message<LEFT_LABELINGS, RIGHT_LABELINGS, INDICES...> (labeling_list_factor.hxx:346)."""
    left_labelings: tuple
    right_labelings: tuple
    indices: tuple
    kind: int = M.M_LABELING


@dataclass(frozen=True)
class test_message:
    """min-normalised copy (reference test/test_model.hxx:66-98)."""
    kind: int = M.M_MINNORM


# ---- containers and FMC ----------------------------------------------------------------------------------
@dataclass
class FactorContainer:
    """FactorContainer<FACTOR_TYPE, FMC, FACTOR_NO, COMPUTE_PRIMAL_SOLUTION=false>"""
    factor_type: type
    factor_no: int
    compute_primal: bool = False


@dataclass
class MessageContainer:
    """MessageContainer<MSG, LEFT_NO, RIGHT_NO, message_passing_schedule, NO_LEFT, NO_RIGHT, FMC, MSG_NO>"""
    message_type: object
    left_factor_no: int
    right_factor_no: int
    schedule: int
    no_left_factors: int
    no_right_factors: int
    message_no: int


class FMC:
    def __init__(self, name: str, FactorList: List[FactorContainer], MessageList: List[MessageContainer]):
        self.name, self.FactorList, self.MessageList = name, list(FactorList), list(MessageList)
        for i, f in enumerate(self.FactorList):
            if f.factor_no != i:
                raise RuntimeError("FactorList: factor numbers must be consecutive")
            if not hasattr(f.factor_type, "kind"):
                raise RuntimeError(f"factor type {f.factor_type!r} has no device kind: only the device-capable "
                                   "factor ops can be plugged in (no CPU fallback)")
        for i, m in enumerate(self.MessageList):
            if m.message_no != i:
                raise RuntimeError("MessageList: message numbers must be consecutive")
            if not hasattr(m.message_type, "kind"):
                raise RuntimeError(f"message type {m.message_type!r} has no device kind")


class LPReparametrizationMode:
    Anisotropic, Anisotropic2, Uniform, DampedUniform, Mixed, Undefined = 0, 1, 2, 3, 4, 5


def LPReparametrizationModeConvert(s: str) -> int:
    if s not in M.REPAM_NAMES:
        raise RuntimeError("reparametrization mode " + s + " unknown")   # reference config.hxx:88
    return M.REPAM_NAMES[s]


class LP:
    """LP<FMC> for the sweep path.  Structural calls are collected on the host; the model is flattened and
    uploaded lazily by the first call that needs the device (everything the reference does after
    set_flags_dirty(), LP_MP.h:1623)."""

    REPARAMETRIZATION_TYPES = {"shared": 0, "residual": 1, "partition": 2, "overlapping_partition": 3, "adaptive": 4}

    def __init__(self, fmc: FMC, device: int = 0, reparametrizationType: str = "shared", innerIteration: int = 5, speculation: int = 16):
        """reparametrizationType / innerIteration: the reference's --reparametrizationType and --innerIteration
        (LP_MP.h:589-593); all five types run on the device.  speculation: how many passes the engine may run ahead of a
        Solve loop that asks for one pass and one bound per iteration (Engine.set_speculation; results unchanged)."""
        self._speculation = int(speculation)
        if reparametrizationType not in self.REPARAMETRIZATION_TYPES:
            raise RuntimeError("reparametrization type " + reparametrizationType + " unknown")
        self._rtype = self.REPARAMETRIZATION_TYPES[reparametrizationType]
        self.FMC = fmc
        self._device = device
        self._factors = []       # (container, op)
        self._messages = []      # (container, left, right)
        self._rel_fwd, self._rel_bwd = [], []
        self._partition_graph = []
        self._inner = int(innerIteration)
        self._tables = {}
        self._shared_tables: List[np.ndarray] = []
        self._constant = 0.0
        self._repam = LPReparametrizationMode.Undefined
        self._engine: Optional[Engine] = None
        self._dirty = True
        self._begun = False
        self._duals_host: Optional[np.ndarray] = None
        self._table_precision = None
        self._pool_changed = False           # set_shared_table / set_diff_table since the last upload
        self._window_sets = {}               # move_windows: the prepared set of a handle list, for the model that is uploaded

    def set_table_precision(self, precision):
        """"f64" / "f32" (strict) / "f32_round": dense pairwise tables as floats on the device, widened in the load, all arithmetic
        in double (Engine.upload, table_precision).  To be called before the first pass: afterwards the model is on the device."""
        if self._engine is not None and not self._dirty:
            raise RuntimeError("set_table_precision: the model is on the device already (call it before the first pass)")
        self._table_precision = precision

    # -- problem construction (reference LP_MP.h:239-285, :698-702) ---------------------------------------
    def add_shared_table(self, table) -> int:
        """a pairwise table [d0, d1] for shared_pairwise_factor ops; returns its id"""
        table = np.array(table, np.float64)
        if table.ndim != 2:
            raise RuntimeError("add_shared_table: a [d0, d1] table is expected")
        self._shared_tables.append(table)
        self._dirty = True
        return len(self._shared_tables) - 1

    def add_diff_table(self, D) -> int:
        """a difference vector for diff_pairwise_factor ops (d0 + d1 - 1 entries) or diff_shift_pairwise_factor ops (any length);
        returns its id in the pool it shares with add_shared_table"""
        D = np.array(D, np.float64)
        if D.ndim != 1 or D.shape[0] < 1:
            raise RuntimeError("add_diff_table: a vector is expected")
        self._shared_tables.append(D.reshape(1, -1))
        self._dirty = True
        return len(self._shared_tables) - 1

    def _set_pool_entry(self, who: str, t: int, values: np.ndarray):
        if not 0 <= int(t) < len(self._shared_tables):
            raise RuntimeError("%s: table id out of range" % who)
        have = self._shared_tables[int(t)]
        if values.shape != have.shape:
            raise RuntimeError("%s: entry %d is %s, not %s (a structural change: another pool is another model)" % (who, t, have.shape, values.shape))
        if np.any(np.isnan(values)):
            raise RuntimeError("%s: NaN entry" % who)
        have[...] = values                   # in place: every factor object bound to the entry sees the new values
        self._pool_changed = True

    def set_shared_table(self, t: int, V):
        """new values for pool entry ``t`` (add_shared_table), same shape.  NOT a structural call: ``upload_costs()`` hands the pool
        to the planned model (Engine.upload_shared_pool).  Every shared_pairwise_factor on the entry sees the new table."""
        V = np.array(V, np.float64)
        if V.ndim != 2:
            raise RuntimeError("set_shared_table: a [d0, d1] table is expected")
        self._set_pool_entry("set_shared_table", t, V)

    def set_diff_table(self, t: int, D):
        """new values for the difference vector ``t`` (add_diff_table), same length; as ``set_shared_table``"""
        D = np.array(D, np.float64)
        if D.ndim != 1:
            raise RuntimeError("set_diff_table: a vector is expected")
        self._set_pool_entry("set_diff_table", t, D.reshape(1, -1))

    def add_factor(self, container: FactorContainer, *args) -> int:
        """a factor of the container: the arguments of ``container.factor_type``, or one ready instance of it.  ONE exception to
        "an instance of the container's type": a ready ``diff_pairwise_factor`` or ``diff_shift_pairwise_factor`` is also taken by
        a container whose factor type is another tabled pairwise kind (PairwiseSimplexFactor, shared_pairwise_factor, the other
        difference-indexed one) — they have one dual layout and
        take the same messages, and the UAI reader (``diff_tables=True``) puts Toeplitz tables into the file's one pairwise
        container this way.  Nothing else crosses types."""
        tabled = (M.F_PAIRWISE_DENSE, M.F_PAIRWISE_SHARED, M.F_PAIRWISE_DIFF, M.F_PAIRWISE_DIFF_SHIFT)     # interchangeable in a container: dual = m1[dim1], m2[dim2]
        ready = len(args) == 1 and (isinstance(args[0], container.factor_type) or
                                    (isinstance(args[0], (diff_pairwise_factor, diff_shift_pairwise_factor)) and getattr(container.factor_type, "kind", None) in tabled))
        op = args[0] if ready else container.factor_type(*args)
        if getattr(op, "kind", None) == M.F_PAIRWISE_SHARED:
            if not 0 <= op.table_id < len(self._shared_tables):
                raise RuntimeError("shared_pairwise_factor: table id out of range (LP.add_shared_table first)")
            op.table = self._shared_tables[op.table_id]
        if getattr(op, "kind", None) == M.F_PAIRWISE_DIFF:
            if not 0 <= op.table_id < len(self._shared_tables) or self._shared_tables[op.table_id].shape != (1, op.dim1 + op.dim2 - 1):
                raise RuntimeError("diff_pairwise_factor: no difference vector of dim1 + dim2 - 1 entries under this id (LP.add_diff_table first)")
            op.vec = self._shared_tables[op.table_id][0]
        if getattr(op, "kind", None) == M.F_PAIRWISE_DIFF_SHIFT:
            if not 0 <= op.table_id < len(self._shared_tables) or self._shared_tables[op.table_id].shape[0] != 1:
                raise RuntimeError("diff_shift_pairwise_factor: no difference vector under this id (LP.add_diff_table first)")
            op.vec = self._shared_tables[op.table_id][0]
        self._pull_duals()
        self._factors.append((container, op))
        self._dirty = True
        return len(self._factors) - 1

    def add_message(self, container: MessageContainer, left: int, right: int) -> int:
        lf, rf = self._factors[left][0], self._factors[right][0]
        if lf.factor_no != container.left_factor_no or rf.factor_no != container.right_factor_no:
            raise RuntimeError("add_message: factor types do not match the message container")
        self._pull_duals()
        self._messages.append((container, left, right))
        self._dirty = True
        return len(self._messages) - 1

    def AddFactorRelation(self, f1: int, f2: int):
        self.ForwardPassFactorRelation(f1, f2)
        self.BackwardPassFactorRelation(f2, f1)

    def ForwardPassFactorRelation(self, f1: int, f2: int):
        self._rel_fwd.append((f1, f2)); self._dirty = True

    def BackwardPassFactorRelation(self, f1: int, f2: int):
        self._rel_bwd.append((f1, f2)); self._dirty = True

    def suggested_order(self, seed: int = 0):
        """the order the engine suggests for this LP as it stands (lpmp_plan_suggest_order on the host-only plan: no GPU needed):
        (by_rank, n_colours) with by_rank[i] = the factor (add_factor's return value) at position i — the updated factors colour by
        colour, one dependent level per colour.  apply_suggested_order() replaces the relations with it."""
        from .engine import Plan
        rank, k = Plan(self.flat_model()).suggest_order(seed)
        by_rank = np.empty(rank.shape[0], np.int64)
        by_rank[rank] = np.arange(rank.shape[0])
        return by_rank.tolist(), k

    def apply_suggested_order(self, seed: int = 0) -> int:
        """drop this LP's factor relations and chain all factors in the suggested order instead — AddFactorRelation(by_rank[i],
        by_rank[i + 1]), what INTEGRATION.md 2a shows a C++ caller doing: same factors, messages and costs, another (equally valid)
        sweep order with far fewer dependent levels for LPs inserted row by row / chain by chain.  Returns the number of colours."""
        by_rank, k = self.suggested_order(seed)
        self._rel_fwd, self._rel_bwd = [], []
        for a, b in zip(by_rank[:-1], by_rank[1:]):
            self.AddFactorRelation(a, b)
        return k

    def put_in_same_partition(self, f1: int, f2: int):
        """reference LP_MP.h:465"""
        self._partition_graph.append((f1, f2)); self._dirty = True

    def GetNumberOfFactors(self) -> int:
        return len(self._factors)

    def GetNumberOfMessages(self) -> int:
        return len(self._messages)

    def GetFactor(self, i: int):
        return self._factors[i][1]

    def add_to_constant(self, x: float):
        self._constant += float(x); self._dirty = True

    def Begin(self):
        self._repam = LPReparametrizationMode.Undefined      # reference LP_MP.h:707
        self._begun = True

    def End(self):
        pass

    def set_reparametrization(self, r):
        self._repam = LPReparametrizationModeConvert(r) if isinstance(r, str) else int(r)

    # -- flattening --------------------------------------------------------------------------------------
    def _table_id(self, msg_op: labeling_message) -> int:
        key = (msg_op.left_labelings, msg_op.right_labelings, msg_op.indices)
        return self._tables.setdefault(key, len(self._tables))

    def flat_model(self) -> M.FlatModel:
        fmc = self.FMC
        self._tables = {}
        mtypes = []
        for mc in fmc.MessageList:
            op = mc.message_type
            param = op.side if op.kind == M.M_UNARY_PAIRWISE else (self._table_id(op) if op.kind == M.M_LABELING else 0)
            mtypes.append(M.MsgType(mc.left_factor_no, mc.right_factor_no, mc.schedule, mc.no_left_factors,
                                    mc.no_right_factors, op.kind, param, getattr(op, "flags", 0)))
        b = M.ModelBuilder(len(fmc.FactorList), mtypes, [int(f.compute_primal) for f in fmc.FactorList])
        for key, _ in sorted(self._tables.items(), key=lambda kv: kv[1]):
            b.add_labeling_table(*key)
        for t in self._shared_tables:
            b.add_shared_table(t)
        for c, op in self._factors:
            if op.kind == M.F_PAIRWISE_SHARED:
                b.add_shared_pairwise(c.factor_no, [op.table_id], [op.scale])
            elif op.kind == M.F_PAIRWISE_DIFF:
                b.add_diff_pairwise(c.factor_no, op.dim1, op.dim2, [op.table_id], [op.scale])
            elif op.kind == M.F_PAIRWISE_DIFF_SHIFT:
                b.add_diff_shift_pairwise(c.factor_no, op.dim1, op.dim2, [op.table_id], [op.scale], [op.shift])
            elif op.kind == M.F_VECTOR:
                b.add_vector_factors(c.factor_no, op.cost[None, :], implicit_origin=op.implicit_origin)
            elif op.kind == M.F_PAIRWISE_DENSE:
                b.add_dense_pairwise(c.factor_no, op.table[None])
            else:
                b.add_potts_pairwise(c.factor_no, op.dim, [op.diff])
        for mc, l, r in self._messages:
            b.add_messages(mc.message_no, l, r)
        if self._rel_fwd:
            a = np.asarray(self._rel_fwd, np.int32); b.add_forward_relations(a[:, 0], a[:, 1])
        if self._rel_bwd:
            a = np.asarray(self._rel_bwd, np.int32); b.add_backward_relations(a[:, 0], a[:, 1])
        if self._partition_graph:
            a = np.asarray(self._partition_graph, np.int32); b.put_in_same_partition(a[:, 0], a[:, 1])
        b.constant = self._constant
        m = b.finish()
        self._flat_costs = m.dual_data               # the costs alone, in dual layout: what upload_costs(warm) takes differences to
        if self._duals_host is not None:     # duals of factors that existed before a structural change
            m.dual_data = m.dual_data.copy()
            n = min(self._duals_host.shape[0], m.dual_data.shape[0])
            m.dual_data[:n] = self._duals_host[:n]
        return m

    # -- new costs on the structure that is on the device (Engine.upload_costs: nothing is planned again) -----------------
    def set_factor_cost(self, i: int, *cost):
        """replace the cost of factor ``i``: the arguments of the factor's own constructor (or one ready instance of its type), as
        ``add_factor`` takes them.  NOT a structural call — the LP stays clean and ``upload_costs()`` hands the new numbers to the
        planned model.  Raises when the kind, a dimension or the pool entry of the factor would change."""
        c, old = self._factors[i]
        new = cost[0] if len(cost) == 1 and isinstance(cost[0], type(old)) else type(old)(*cost)
        if new.kind != old.kind:
            raise RuntimeError("set_factor_cost: the kind of factor %d would change" % i)
        if old.kind == M.F_VECTOR:
            same = new.cost.shape == old.cost.shape and new.implicit_origin == old.implicit_origin
        elif old.kind == M.F_PAIRWISE_DENSE:
            same = (new.dim1, new.dim2) == (old.dim1, old.dim2)
        elif old.kind == M.F_PAIRWISE_POTTS:
            same = new.dim == old.dim
        elif old.kind == M.F_PAIRWISE_SHARED:
            same = new.table_id == old.table_id          # (the pool is structure: another table is another model)
            new.table = old.table
        else:
            same = (new.table_id, new.dim1, new.dim2) == (old.table_id, old.dim1, old.dim2)
            new.vec = old.vec
        if not same:
            raise RuntimeError("set_factor_cost: the shape of factor %d would change (a structural change: add the factor to a new LP)" % i)
        self._factors[i] = (c, new)

    def upload_costs(self, warm: bool = False):
        """hand the factors' current costs (``set_factor_cost``) to the device.  No structural call since the last upload: the
        planned model gets new numbers (Engine.upload_costs), every schedule stays.  Cold (default): constants, and duals = the
        costs — a fresh problem.  ``warm``: constants only, the messages are kept, and every unary whose cost changed receives
        new - old (Engine.set_vectors, accumulate): the reparametrised problem of the new costs; of the pairwise factors only those
        whose constants differ from the uploaded ones are sent (Engine.set_constants).  A pool changed by ``set_shared_table`` /
        ``set_diff_table`` goes first (Engine.upload_shared_pool).  After a structural call this is the ordinary upload."""
        if self._engine is None or self._dirty:
            self._ready()
            return
        e = self._ready()
        kept, self._duals_host = self._duals_host, None      # (flat_model lays pulled duals over the costs: not wanted here)
        try:
            new = self.flat_model()
        finally:
            self._duals_host = kept
        if self._pool_changed:
            e.upload_shared_pool(new.sh_data)
            self._pool_changed = False
        if warm:
            listed = getattr(e, "set_constants", None)     # (an engine object without listed constants takes the whole array)
            if new.const_data.shape[0] > 0 and listed is None:
                e.upload_costs(const=new.const_data)
            elif new.const_data.shape[0] > 0:
                coff = new.const_offsets()
                diff = new.const_data != self._model.const_data
                pw = [int(f) for f in np.flatnonzero(new.f_kind != M.F_VECTOR) if np.any(diff[coff[f]:coff[f + 1]])]
                if pw:
                    rows = np.zeros((len(pw), int(max(coff[f + 1] - coff[f] for f in pw))))
                    for k, f in enumerate(pw):
                        rows[k, :coff[f + 1] - coff[f]] = new.const_data[coff[f]:coff[f + 1]]
                    listed(pw, rows)
            off = new.dual_offsets()
            delta = new.dual_data - self._cost_dual    # new - old COSTS (the device holds reparametrised duals; so may _model)
            vec = np.flatnonzero(new.f_kind == M.F_VECTOR)
            changed = [int(f) for f in vec if np.any(delta[off[f]:off[f + 1]] != 0.0)]
            if changed:
                src = np.zeros((len(changed), int(max(off[f + 1] - off[f] for f in changed))))
                for k, f in enumerate(changed):
                    src[k, :off[f + 1] - off[f]] = delta[off[f]:off[f + 1]]
                e.set_vectors(changed, src, accumulate=True)
        else:
            e.upload_costs(const=new.const_data if new.const_data.shape[0] > 0 else None, duals=new.dual_data)
        self._model = new
        self._cost_dual = new.dual_data
        e.model = new

    def move_windows(self, handles, delta, new_costs=None, carry_labels=False):
        """move the label windows of the unaries ``handles`` (add_factor's return values, each once) by ``delta[i]`` labels ON THE
        DEVICE (Engine.window_set / WindowSet.move): new label x of unary i is its old label x + delta[i], theta and the messages of
        the adjacent ``diff_shift_pairwise_factor``s are carried along their label axis, and the shift of every such factor becomes
        shift + delta_left - delta_right — the warm start that belongs to the new windows.  ``new_costs[i]``: the unary's cost in
        its new window (same length); None: labels that stay keep their cost and labels that enter the window copy the nearest end.
        The stored ops follow (``shift`` of the adjacent factors, the unaries' ``cost``), so a following ``upload_costs(warm=True)``
        finds nothing to send.  NOT a structural call: every schedule stays.  Every message of a listed unary must lead to a
        diff_shift_pairwise_factor (Engine.window_set raises otherwise, naming the factor).  ``carry_labels``: the labels move with
        their windows (label x becomes x - delta[i], clamped into the window) instead of becoming unset."""
        import dataclasses
        e = self._ready()
        handles = [int(h) for h in handles]
        delta = np.asarray(delta).reshape(-1)
        if delta.shape[0] != len(handles) or (len(handles) and not np.issubdtype(delta.dtype, np.integer)):
            raise RuntimeError("move_windows: one integer delta per handle")
        if new_costs is not None and len(new_costs) != len(handles):
            raise RuntimeError("move_windows: one cost vector per handle")
        key = tuple(handles)
        if key not in self._window_sets:                  # (prepared once per list and upload: _ready drops them with the model)
            self._window_sets[key] = (e.window_set(handles), M.window_links(self._model, handles)[2])
        ws, pairs = self._window_sets[key]
        old, new = [], []
        for i, h in enumerate(handles):
            c = self._factors[h][1].cost
            g = np.clip(np.arange(c.shape[0]) + int(delta[i]), 0, c.shape[0] - 1)
            n = c[g] if new_costs is None else np.asarray(new_costs[i], np.float64).reshape(-1)
            if n.shape != c.shape:
                raise RuntimeError("move_windows: the cost of factor %d would change its length (a structural change)" % h)
            old.append(c); new.append(np.array(n, copy=True))
        kw = {"carry_labels": True} if carry_labels else {}
        if new_costs is None:
            ws.move(delta, **kw)
        else:
            L = max(ws.max_labels, 1)
            co, cn = np.zeros((len(handles), L)), np.zeros((len(handles), L))
            for i in range(len(handles)):
                co[i, :old[i].shape[0]] = old[i]; cn[i, :new[i].shape[0]] = new[i]
            ws.move(delta, cost_old=co, cost_new=cn, **kw)
        # the host's books: ops, the uploaded constants and the costs the next warm upload takes differences to
        const = np.array(self._model.const_data, np.float64, copy=True)
        coff, doff = self._model.const_offsets(), self._model.dual_offsets()
        for p, lrow, rrow in pairs:
            d = (int(delta[lrow]) if lrow >= 0 else 0) - (int(delta[rrow]) if rrow >= 0 else 0)
            if d:
                op = self._factors[p][1]
                op.shift = int(min(max(op.shift + d, -M.DIFF_SHIFT_MAX), M.DIFF_SHIFT_MAX))
                const[coff[p] + 1] = np.float64(op.shift)
        cost_dual = np.array(self._cost_dual, np.float64, copy=True)
        for i, h in enumerate(handles):
            self._factors[h][1].cost = new[i]
            cost_dual[doff[h]:doff[h + 1]] = new[i]
        self._model = dataclasses.replace(self._model, const_data=const, _keep=[])
        self._cost_dual = cost_dual
        e.model = self._model

    def _pull_duals(self):
        if self._engine is not None and not self._dirty:
            self._duals_host = self._engine.download_duals()

    def _ready(self) -> Engine:
        if len(self._factors) <= 1:
            raise RuntimeError("LP needs more than one factor")           # reference assert, LP_MP.h:708
        if self._engine is None:
            self._engine = Engine(self._device)
            self._engine.set_speculation(self._speculation)
        if self._dirty:
            self._model = self.flat_model()
            self._cost_dual = self._flat_costs       # (not _model.dual_data: after a structural call that holds pulled duals)
            self._engine.upload(self._model, table_precision=self._table_precision)
            self._dirty = False
            self._window_sets = {}
            self._pool_changed = False
        self._engine.set_inner_iterations(self._inner)
        self._engine.set_reparametrization_type(self._rtype)
        return self._engine

    # -- the hot path ---------------------------------------------------------------------------------------
    def _mode(self) -> int:
        if self._repam == LPReparametrizationMode.Undefined:
            raise RuntimeError("no reparametrization mode set")           # reference LP_MP.h:458
        return self._repam

    def ComputePass(self, iteration=0, *rows):
        """ComputePass(iteration)  or  ComputePass(factors, (omega_off, omega), (mask_off, mask))."""
        e = self._ready()
        if rows:
            factors = iteration
            (om_off, om), (mk_off, mk) = rows
            e.compute_pass_custom(factors, om_off, om, mk_off, mk)
            return
        e.set_reparametrization(self._mode())
        e.compute_pass(1)

    def ComputePasses(self, n: int):
        """n consecutive passes in one call: same results as n x ComputePass, the engine joins them"""
        if n > 0:
            e = self._ready(); e.set_reparametrization(self._mode()); e.compute_pass(int(n))

    def ComputeForwardPass(self):
        e = self._ready(); e.set_reparametrization(self._mode()); e.forward_pass()

    def ComputeBackwardPass(self):
        e = self._ready(); e.set_reparametrization(self._mode()); e.backward_pass()

    def LowerBound(self, dst_dev=None):
        """``dst_dev``: a raw device pointer to one double — written asynchronously on the engine's stream without any host
        synchronisation (Engine.lower_bound); returns None then"""
        return self._ready().lower_bound(dst_dev)

    # -- primal rounding inside the sweep (reference LP_MP.h:914-940, 1067-1082, 1521-1536) ------------------
    def ComputeForwardPassAndPrimal(self, iteration: int):
        e = self._ready(); e.set_reparametrization(self._mode()); e.forward_pass_and_primal(iteration)

    def ComputeBackwardPassAndPrimal(self, iteration: int):
        e = self._ready(); e.set_reparametrization(self._mode()); e.backward_pass_and_primal(iteration)

    def ComputePassAndPrimal(self, iteration: int):
        self.ComputeForwardPassAndPrimal(iteration)
        self.ComputeBackwardPassAndPrimal(iteration)

    def CheckPrimalConsistency(self) -> bool:
        return self._ready().check_primal_consistency()

    def EvaluatePrimal(self, dst_dev=None):
        """``dst_dev``: as in ``LowerBound``"""
        return self._ready().evaluate_primal(dst_dev)

    def decode_primal(self, direction: int = 0, refine: int = 0) -> float:
        """labels from the current duals by conditional rounding (Engine.decode_primal; no reference counterpart):
        reads the duals only, returns EvaluatePrimal(); primal() then returns the labels.  Decode against the direction of the
        last sweep: forward (0) after ComputePass."""
        e = self._ready()
        e.decode_primal(direction, refine)
        return e.evaluate_primal()

    def path_moves(self, groups, rounds: int = 1) -> float:
        """exact relabelling of whole paths given all other labels (Engine.path_set / PathSet.move; no reference
        counterpart): ``groups`` is a sequence of groups, each a sequence of paths, each a sequence of vector-factor handles (what
        ``add_factor`` returned) whose consecutive members share exactly one pairwise factor.  Runs the groups in order ``rounds``
        times on the labels the primal array holds (after ``decode_primal``, say) and returns EvaluatePrimal(); on a complete
        labelling that cost never rises.  The prepared set is made and closed here: keep ``Engine.path_set`` for repeated moves."""
        e = self._ready()
        ps = e.path_set(groups)
        try:
            ps.move(rounds)
            return e.evaluate_primal()
        finally:
            ps.close()

    def forest_moves(self, groups=None, rounds: int = 1) -> float:
        """exact relabelling of induced forests given all other labels (Engine.forest_set / ForestSet.move; no
        reference counterpart): ``groups`` is a sequence of (unaries, parent) pairs of vector-factor handles, parent[i] the handle
        of the parent of unaries[i] or -1 for a root; None takes the cover the engine suggests for this LP
        (``Plan.suggest_forests``), which any graph has.  Runs the groups in order ``rounds`` times on the labels the primal array
        holds and returns EvaluatePrimal(); on a complete labelling that cost never rises.  The prepared set is made and closed
        here: keep ``Engine.forest_set`` for repeated moves."""
        e = self._ready()
        if groups is None:
            groups = e.plan.suggest_forests()
        fs = e.forest_set(groups)
        try:
            fs.move(rounds)
            return e.evaluate_primal()
        finally:
            fs.close()

    def readout(self, factor_handles=None):
        """a prepared read-out (Engine.readout; no reference counterpart) of the listed vector factors — what
        ``add_factor`` returned for them, None: all of them — with ``labels()``, ``vectors()`` and ``beliefs()`` into host or device
        arrays, and ``set_labels()`` from one (the start labelling of ``path_moves`` / ``forest_moves``).  It belongs to the uploaded model: a structural change of the LP (the next upload) ends it."""
        return self._ready().readout(factor_handles)

    def primal(self) -> np.ndarray:
        """[n_factors, 2] the factors' primal_ members in serialize_primal order: vector factor (label, 0), pairwise
        factor (x0, x1); an unset entry holds the dimension."""
        return self._ready().download_primal()

    def get_omega(self):
        """omega_storage{forward, backward, receive_mask_forward, receive_mask_backward} as CSR pairs."""
        p = self._ready().plan
        m = self._mode()
        return {"forward": p.omega(0, m), "backward": p.omega(1, m),
                "receive_mask_forward": p.mask(0, m), "receive_mask_backward": p.mask(1, m)}

    def forward_update_ordering(self):
        return self._ready().plan.update_order(0)

    def backward_update_ordering(self):
        return self._ready().plan.update_order(1)

    def duals(self) -> np.ndarray:
        """packed duals in serialize_dual order (reference factors_messages.hxx:3196-3223)."""
        return self._ready().download_duals()


# ---- caller loop --------------------------------------------------------------------------------------------
@dataclass
class LpControl:
    repam: int = LPReparametrizationMode.Undefined
    computePrimal: bool = False
    computeLowerBound: bool = False
    tighten: bool = False
    end: bool = False
    error: bool = False


class StandardVisitor:
    """reference include/visitors/standard_visitor.hxx; same option names and defaults (:32-44)."""

    def __init__(self, maxIter=1000, timeout=None, primalComputationInterval=5, primalComputationStart=1,
                 lowerBoundComputationInterval=1, minDualImprovement=None, minDualImprovementInterval=10,
                 standardReparametrization="anisotropic", roundingReparametrization="damped_uniform", verbosity=0):
        self.maxIter, self.timeout = maxIter, timeout
        self.primalComputationInterval, self.primalComputationStart = primalComputationInterval, primalComputationStart
        self.lowerBoundComputationInterval = lowerBoundComputationInterval
        self.minDualImprovement, self.minDualImprovementInterval = minDualImprovement, minDualImprovementInterval
        self.standardReparametrization = LPReparametrizationModeConvert(standardReparametrization)
        self.roundingReparametrization = LPReparametrizationModeConvert(roundingReparametrization)
        self.verbosity = verbosity
        self.lowerBound_: List[float] = []

    def begin(self, lp) -> LpControl:
        self.remainingIter = self.maxIter
        self.curIter = 0
        self.beginTime = time.monotonic()
        return LpControl(repam=self.standardReparametrization, computeLowerBound=True)

    def visit(self, c: LpControl, lowerBound: float, primalBound: float) -> LpControl:
        self.lowerBound_.append(lowerBound)
        elapsed = time.monotonic() - self.beginTime
        if self.verbosity >= 1 and (c.computePrimal or c.computeLowerBound):
            print(f"iteration = {self.curIter}, lower bound = {lowerBound}, time elapsed = {elapsed:.2f}s")
        self.curIter += 1
        self.remainingIter -= 1
        ret = LpControl()
        if self.remainingIter == 0:
            ret.end = True
            return ret
        if primalBound <= lowerBound + 1e-8:
            ret.end = True
            return ret
        if self.timeout is not None and elapsed >= self.timeout:
            self.remainingIter = min(1, self.remainingIter)
        # (reference standard_visitor.hxx:163-165 starts one visit earlier and then indexes out of bounds; see LP_gpu.hxx)
        if (c.computeLowerBound and len(self.lowerBound_) > self.minDualImprovementInterval and self.minDualImprovement is not None):
            prev = self.lowerBound_[len(self.lowerBound_) - 1 - self.minDualImprovementInterval]
            if self.minDualImprovement > 0 and lowerBound - prev < self.minDualImprovement:
                self.remainingIter = min(1, self.remainingIter)
        if self.remainingIter == 1:
            ret.computePrimal = True
            ret.computeLowerBound = True
            ret.repam = self.roundingReparametrization
            return ret
        ret.repam = self.standardReparametrization
        if self.curIter >= self.primalComputationStart and (self.curIter - self.primalComputationStart) % self.primalComputationInterval == 0:
            ret.computePrimal = True
            ret.repam = self.roundingReparametrization
        if self.curIter % self.lowerBoundComputationInterval == 0:
            ret.computeLowerBound = True
        return ret

    def quiet_iterations(self, c: LpControl) -> int:
        """how many iterations from now on (this one included) ask for neither a lower bound nor a primal: the solver
        may run them as ONE device call and replay the visits afterwards (LP_gpu_solver.hxx has the same rule)"""
        if c.end or c.error or c.computeLowerBound or c.computePrimal or self.timeout is not None:
            return 1
        n = 1
        for j in range(1, max(1, self.remainingIter - 1)):
            it = self.curIter + j
            if self.remainingIter - j <= 1:
                break
            if it >= self.primalComputationStart and (it - self.primalComputationStart) % self.primalComputationInterval == 0:
                break
            if it % self.lowerBoundComputationInterval == 0:
                break
            n += 1
        return n

    def end(self, lower_bound: float, upper_bound: float):
        if self.verbosity >= 1:
            print(f"final lower bound = {lower_bound}, upper bound = {upper_bound}")


class Solver:
    """Solver<LP_TYPE, VISITOR>::Solve with its PreIterate / Iterate / PostIterate / RegisterPrimal hooks (reference
    include/solver.hxx:230-337).  The base class never rounds (bestPrimalCost_ stays +inf unless a derived solver
    registers a primal); the visitor still switches to the rounding reparametrisation where the reference would."""

    def __init__(self, lp: LP, visitor: Optional[StandardVisitor] = None):
        self.lp_ = lp
        self.visitor_ = visitor or StandardVisitor()
        self.lowerBound_ = -np.inf
        self.bestPrimalCost_ = np.inf
        self.solution_ = None
        self.iter = 0

    def GetLP(self) -> LP:
        return self.lp_

    def PreIterate(self, c: LpControl):
        self.lp_.set_reparametrization(c.repam)

    def Iterate(self, c: LpControl):
        self.lp_.ComputePass(self.iter)

    def PostIterate(self, c: LpControl):
        if c.computeLowerBound:
            self.lowerBound_ = self.lp_.LowerBound()

    def RegisterPrimal(self):
        """solver.hxx:320-337: keep the labeling if it is cheaper than the best one so far and consistent"""
        cost = self.lp_.EvaluatePrimal()
        if cost < self.bestPrimalCost_ and self.lp_.CheckPrimalConsistency():
            self.bestPrimalCost_ = cost
            self.solution_ = self.lp_.primal()

    def Solve(self) -> int:
        self.lp_.Begin()
        c = self.visitor_.begin(self.lp_)
        while not c.end and not c.error:
            self.PreIterate(c)
            # iterations in which the visitor asks for nothing run as one device call (the engine joins consecutive
            # passes); only for this class and MpRoundingSolver themselves — a subclass may override Iterate
            quiet = 1
            if type(self) in (Solver, MpRoundingSolver) and hasattr(self.visitor_, "quiet_iterations"):
                quiet = self.visitor_.quiet_iterations(c)
            if quiet > 1:
                self.lp_.ComputePasses(quiet)
                for _ in range(quiet):
                    if c.end or c.error:
                        break
                    c = self.visitor_.visit(c, self.lowerBound_, self.bestPrimalCost_)
                    self.iter += 1
                continue
            self.Iterate(c)
            self.PostIterate(c)
            c = self.visitor_.visit(c, self.lowerBound_, self.bestPrimalCost_)
            self.iter += 1
        if not c.error:
            self.lp_.End()
            if self._rounds:
                self.RegisterPrimal()
            self.lowerBound_ = self.lp_.LowerBound()
            self.visitor_.end(self.lowerBound_, self.bestPrimalCost_)
        return int(not c.error)

    _rounds = False   # the reference calls RegisterPrimal after End() in every solver (solver.hxx:247); without a
                      # rounding pass every primal_ is unset and the cost is +inf, so the base class skips the call

    def lower_bound(self) -> float:
        return self.lowerBound_

    def primal_cost(self) -> float:
        return self.bestPrimalCost_


class MpRoundingSolver(Solver):
    """MpRoundingSolver<SOLVER>: local rounding interleaved with message passing (reference include/solver.hxx:380-400).
    On the iterations the visitor marks computePrimal (every --primalComputationInterval-th, and the last one) the
    pass is run as forward-and-primal, register, backward-and-primal, register."""
    _rounds = True

    def Iterate(self, c: LpControl):
        if c.computePrimal:
            self.lp_.ComputeForwardPassAndPrimal(self.iter)
            self.RegisterPrimal()
            self.lp_.ComputeBackwardPassAndPrimal(self.iter)
            self.RegisterPrimal()
        else:
            super().Iterate(c)
