"""Flat factor-graph model: the Python view of ``include/lpmp_model.h``.

``ModelBuilder`` collects what a user of the reference adds through ``LP<FMC>::add_factor`` /
``add_message`` / ``AddFactorRelation`` (reference: include/LP_MP.h:239-285, :698-702) and
``finish()`` packs it into the arrays the C-ABI engine (include/lpmp_engine.h) takes.
Bulk ``add_*`` calls keep insertion order: ids are handed out consecutively, exactly as the
reference appends to ``f_`` / ``m_``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

# enum lpmp_factor_kind
F_VECTOR, F_PAIRWISE_DENSE, F_PAIRWISE_POTTS, F_PAIRWISE_SHARED, F_PAIRWISE_DIFF, F_PAIRWISE_DIFF_SHIFT = 0, 1, 2, 3, 4, 6      # (5 is not assigned)
DIFF_SHIFT_MAX = 1 << 30      # |shift| of a DIFF_SHIFT factor (include/lpmp_model.h)
FF_IMPLICIT_ORIGIN = 1
# enum lpmp_msg_kind
M_UNARY_PAIRWISE, M_LABELING, M_MINNORM = 0, 1, 2
# enum lpmp_schedule (reference include/config.hxx:43-49)
SCHED_LEFT, SCHED_RIGHT, SCHED_FULL, SCHED_ONLY_SEND, SCHED_NONE = 0, 1, 2, 3, 4
# enum lpmp_repam_mode (reference include/config.hxx:71)
REPAM_ANISOTROPIC, REPAM_ANISOTROPIC2, REPAM_UNIFORM, REPAM_DAMPED_UNIFORM, REPAM_MIXED = 0, 1, 2, 3, 4
REPAM_NAMES = {"anisotropic": 0, "anisotropic2": 1, "uniform": 2, "damped_uniform": 3, "mixed": 4}
FORWARD, BACKWARD = 0, 1
# enum lpmp_msg_flags
MF_IMPROVEMENT, MF_BATCH_TO_RIGHT, MF_BATCH_TO_LEFT = 1, 2, 4
# enum lpmp_reparametrization_type (reference --reparametrizationType, LP_MP.h:710-722)
RTYPE_SHARED, RTYPE_RESIDUAL, RTYPE_PARTITION, RTYPE_OVERLAPPING_PARTITION, RTYPE_ADAPTIVE = 0, 1, 2, 3, 4
RTYPE_NAMES = {"shared": 0, "residual": 1, "partition": 2, "overlapping_partition": 3, "adaptive": 4}
# NO_OF_LEFT/RIGHT_FACTORS shorthands (reference include/config.hxx:60-66)
variableMessageNumber = 0
atMostOneMessage, atMostTwoMessages = -1, -2


class c_msg_type(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("left_ftype", "right_ftype", "schedule", "n_left", "n_right", "kind", "param", "flags")]


class c_model(C.Structure):
    _fields_ = [
        ("n_ftypes", C.c_int32), ("ftype_computes_primal", C.c_void_p),
        ("n_mtypes", C.c_int32), ("mtypes", C.c_void_p),
        ("n_tables", C.c_int32), ("tab_off", C.c_void_p), ("tab_data", C.c_void_p), ("tab_nleft", C.c_void_p),
        ("n_factors", C.c_int64), ("f_type", C.c_void_p), ("f_kind", C.c_void_p), ("f_flags", C.c_void_p),
        ("f_dim0", C.c_void_p), ("f_dim1", C.c_void_p), ("const_data", C.c_void_p), ("dual_data", C.c_void_p),
        ("n_messages", C.c_int64), ("m_type", C.c_void_p), ("m_left", C.c_void_p), ("m_right", C.c_void_p),
        ("n_rel_fwd", C.c_int64), ("rel_fwd", C.c_void_p), ("n_rel_bwd", C.c_int64), ("rel_bwd", C.c_void_p),
        ("constant", C.c_double),
        ("n_part_pairs", C.c_int64), ("part_pairs", C.c_void_p),
        ("n_shared_tables", C.c_int32), ("sh_off", C.c_void_p), ("sh_dim0", C.c_void_p), ("sh_dim1", C.c_void_p),
        ("sh_data", C.c_void_p), ("f_table", C.c_void_p),
    ]


@dataclass
class MsgType:
    """One entry of ``FMC::MessageList`` (reference include/factors_messages.hxx:571-578)."""
    left_ftype: int
    right_ftype: int
    schedule: int = SCHED_LEFT
    n_left: int = variableMessageNumber
    n_right: int = 1
    kind: int = M_UNARY_PAIRWISE
    param: int = 0
    flags: int = 0          # MF_* : optional members of the message op (include/lpmp_model.h, enum lpmp_msg_flags)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


@dataclass
class FlatModel:
    n_ftypes: int
    ftype_computes_primal: np.ndarray
    mtypes: List[MsgType]
    tab_off: np.ndarray
    tab_data: np.ndarray
    tab_nleft: np.ndarray
    f_type: np.ndarray
    f_kind: np.ndarray
    f_flags: np.ndarray
    f_dim0: np.ndarray
    f_dim1: np.ndarray
    const_data: Optional[np.ndarray]   # None: supplied separately as a device buffer
    dual_data: Optional[np.ndarray]
    m_type: np.ndarray
    m_left: np.ndarray
    m_right: np.ndarray
    rel_fwd: np.ndarray                # [n,2] int32
    rel_bwd: np.ndarray
    constant: float = 0.0
    part_pairs: Optional[np.ndarray] = None   # [n,2] int32: put_in_same_partition(f1, f2) calls in call order
    # shared pairwise tables (F_PAIRWISE_SHARED: cost = scale * V[a][b], the factor's one const double is the scale):
    # table t is sh_dim0[t] x sh_dim1[t], row-major at sh_data[sh_off[t]]; f_table[f] = table of factor f (-1: none).
    # F_PAIRWISE_DIFF: cost = scale * D[a - b + d1 - 1], D = entry f_table[f] of the same pool, a [1, d0 + d1 - 1] table
    # F_PAIRWISE_DIFF_SHIFT: two const doubles {scale, shift}; cost = scale * D[clip(a - b + shift, 0, n - 1)], D a [1, n] entry, any n
    sh_off: Optional[np.ndarray] = None       # [n_tables + 1] int64
    sh_dim0: Optional[np.ndarray] = None      # [n_tables] int32
    sh_dim1: Optional[np.ndarray] = None
    sh_data: Optional[np.ndarray] = None      # float64, host memory always
    f_table: Optional[np.ndarray] = None      # [n_factors] int32, None when no factor is SHARED, DIFF or DIFF_SHIFT
    _keep: list = field(default_factory=list, repr=False)

    def __getstate__(self):          # the ctypes views of c_struct() are per process and rebuilt on demand
        d = dict(self.__dict__)
        d["_keep"] = []
        return d

    @property
    def n_factors(self) -> int:
        return int(self.f_type.shape[0])

    @property
    def n_messages(self) -> int:
        return int(self.m_type.shape[0])

    def const_sizes(self) -> np.ndarray:
        d0 = self.f_dim0.astype(np.int64)
        d1 = self.f_dim1.astype(np.int64)
        return np.where(self.f_kind == F_PAIRWISE_DENSE, d0 * d1, np.where(self.f_kind == F_PAIRWISE_DIFF_SHIFT, 2,
                        np.where((self.f_kind == F_PAIRWISE_POTTS) | (self.f_kind == F_PAIRWISE_SHARED) | (self.f_kind == F_PAIRWISE_DIFF), 1, 0)))

    def dual_sizes(self) -> np.ndarray:
        d0 = self.f_dim0.astype(np.int64)
        d1 = self.f_dim1.astype(np.int64)
        return np.where((self.f_kind == F_PAIRWISE_DENSE) | (self.f_kind == F_PAIRWISE_SHARED) | (self.f_kind == F_PAIRWISE_DIFF) | (self.f_kind == F_PAIRWISE_DIFF_SHIFT), d0 + d1, np.where(self.f_kind == F_PAIRWISE_POTTS, 2 * d0, d0))

    def dual_offsets(self) -> np.ndarray:
        return np.concatenate([[0], np.cumsum(self.dual_sizes())]).astype(np.int64)

    def const_offsets(self) -> np.ndarray:
        return np.concatenate([[0], np.cumsum(self.const_sizes())]).astype(np.int64)

    @property
    def n_shared_tables(self) -> int:
        return 0 if self.sh_dim0 is None else int(self.sh_dim0.shape[0])

    @property
    def has_shared(self) -> bool:
        return bool(np.any(self.f_kind == F_PAIRWISE_SHARED))

    def shared_table(self, t: int) -> np.ndarray:
        """table t of the pool as a [d0, d1] view"""
        d0, d1 = int(self.sh_dim0[t]), int(self.sh_dim1[t])
        return self.sh_data[int(self.sh_off[t]): int(self.sh_off[t]) + d0 * d1].reshape(d0, d1)

    @property
    def has_diff(self) -> bool:
        """any difference-indexed factor, plain (DIFF) or shifted (DIFF_SHIFT)"""
        return bool(np.any((self.f_kind == F_PAIRWISE_DIFF) | (self.f_kind == F_PAIRWISE_DIFF_SHIFT)))

    def _expand(self, which: int, name: str) -> "FlatModel":
        """the factors of kind ``which`` (SHARED, or DIFF: both difference-indexed kinds) replaced by DENSE factors; the pool goes with the last factor
        that uses it.  While factors of the other pooled kind remain, the pool stays WHOLE: the entries that only the expanded
        factors used are kept (``n_shared_tables`` still counts them, an upload still carries them), so that the table ids of
        the remaining factors do not move."""
        import dataclasses
        is_diff = (self.f_kind == F_PAIRWISE_DIFF) | (self.f_kind == F_PAIRWISE_DIFF_SHIFT)
        is_exp = is_diff if which == F_PAIRWISE_DIFF else self.f_kind == F_PAIRWISE_SHARED
        keep_pool = bool(np.any(((self.f_kind == F_PAIRWISE_SHARED) | is_diff) & ~is_exp))
        if keep_pool:
            pool = dict(f_table=np.where(is_exp, np.int32(-1), self.f_table).astype(np.int32), _keep=[])
        else:
            pool = dict(sh_off=None, sh_dim0=None, sh_dim1=None, sh_data=None, f_table=None, _keep=[])
        if not is_exp.any():
            return dataclasses.replace(self, **pool)
        if self.const_data is None:
            raise ValueError(name + ": the model has no host constants")
        old_off = self.const_offsets()
        kind = self.f_kind.copy()
        kind[is_exp] = F_PAIRWISE_DENSE
        new = dataclasses.replace(self, f_kind=kind, **pool)
        new_off = new.const_offsets()
        const = np.empty(int(new_off[-1]), np.float64)
        # runs of factors that stay keep their constants as they are
        f = 0
        nf = self.n_factors
        while f < nf:
            g = f
            if is_exp[f]:
                V = self.shared_table(int(self.f_table[f]))
                if which == F_PAIRWISE_DIFF:
                    d0, d1 = int(self.f_dim0[f]), int(self.f_dim1[f])
                    k = np.arange(d0, dtype=np.int64)[:, None] - np.arange(d1, dtype=np.int64)[None, :]
                    if self.f_kind[f] == F_PAIRWISE_DIFF_SHIFT:     # the clamped index, the shift converted as the device converts it
                        V = V.reshape(-1)[np.clip(k + diff_shift_int(self.const_data[old_off[f] + 1]), 0, V.size - 1)]
                    else:
                        V = V.reshape(-1)[k + (d1 - 1)]
                const[new_off[f]: new_off[f + 1]] = (np.float64(self.const_data[old_off[f]]) * V).reshape(-1)
                f += 1
            else:
                while g < nf and not is_exp[g]:
                    g += 1
                const[new_off[f]: new_off[g]] = self.const_data[old_off[f]: old_off[g]]
                f = g
        new.const_data = const
        return new

    def expand_shared(self) -> "FlatModel":
        """the same model with every SHARED factor replaced by a DENSE factor whose table is ``np.float64(scale) * V`` —
        same factor order, messages, relations and duals (the dual layouts of the two kinds are equal), no pool (it stays while
        DIFF factors use it).  Plain numpy; a model without SHARED factors is returned with its arrays shared."""
        return self._expand(F_PAIRWISE_SHARED, "expand_shared")

    def expand_diff(self) -> "FlatModel":
        """the same model with every DIFF and every DIFF_SHIFT factor replaced by a DENSE factor whose table is
        ``np.float64(scale) * D[a - b + d1 - 1]`` (DIFF_SHIFT: ``D[clip(a - b + diff_shift_int(shift), 0, n - 1)]``) — the yardstick
        of the two kinds, as expand_shared() is for SHARED factors"""
        return self._expand(F_PAIRWISE_DIFF, "expand_diff")

    def with_f32_tables(self) -> "FlatModel":
        """the same model with every entry of a DENSE pairwise table rounded to float32 (nearest even) and widened again —
        the model an engine with ``table_precision="f32_round"`` computes on, bit for bit, and the yardstick of both f32 modes.
        Potts scalars, SHARED / DIFF scales, the shared pool and the duals are untouched (shared with ``self``); a model whose
        tables are float-valued already comes back with equal values."""
        import dataclasses
        if self.const_data is None:
            raise ValueError("with_f32_tables: the model has no host constants")
        off = self.const_offsets()
        dense = np.repeat(self.f_kind == F_PAIRWISE_DENSE, np.diff(off))
        const = np.array(self.const_data, np.float64, copy=True)
        with np.errstate(over="ignore"):
            const[dense] = const[dense].astype(np.float32).astype(np.float64)
        return dataclasses.replace(self, const_data=const, _keep=[])

    def with_pool(self, sh_data) -> "FlatModel":
        """the same structure with other VALUES in the shared pool (``sh_data`` packed as ``self.sh_data``: same entries, same
        dims) — what ``Engine.upload_shared_pool`` / ``Plan.set_shared_pool`` turn a planned model into.  Another length and a NaN
        entry are refused; every other array is shared with ``self``."""
        import dataclasses
        if self.sh_data is None:
            raise ValueError("with_pool: the model has no shared pool")
        sh = np.array(sh_data, np.float64, copy=True).reshape(-1)
        if sh.shape != np.shape(self.sh_data):
            raise ValueError(f"with_pool: a pool of {np.shape(self.sh_data)[0]} entries expected, got {sh.shape[0]}")
        if np.any(np.isnan(sh)):
            raise ValueError("with_pool: NaN entry")
        return dataclasses.replace(self, sh_data=sh, _keep=[])

    def with_factor_order(self, rank: np.ndarray) -> "FlatModel":
        """the same factors, messages and costs with the factor relations REPLACED by a chain through all factors in the order
        ``rank[f]`` (position of factor f, e.g. Plan.suggest_order): AddFactorRelation(by_rank[i], by_rank[i + 1]) for consecutive
        positions (reference LP_MP.h:698-702: forward sweep in that order, backward sweep in the reverse one; the chain is the only
        topological order, so no tie is left to the sort) — what INTEGRATION.md 2a shows a C++ caller doing with
        lpmp_plan_suggest_order's answer.  Arrays are shared with ``self``."""
        import dataclasses
        rank = np.asarray(rank, np.int64)
        by_rank = np.empty(rank.shape[0], np.int32)
        by_rank[rank] = np.arange(rank.shape[0], dtype=np.int32)
        fwd = np.ascontiguousarray(np.stack([by_rank[:-1], by_rank[1:]], 1))
        return dataclasses.replace(self, rel_fwd=fwd, rel_bwd=np.ascontiguousarray(fwd[:, ::-1]), _keep=[])

    def dump(self, path: str):
        """the model as one flat binary file in the order of include/lpmp_model.h — what the C++ hosts read
        (lp_mp_amd/include/lpmp_lockstep.hxx, model_file; tools/mgpu_rccl_driver.cpp --model-file)"""
        if self.dual_data is None:
            raise ValueError("dump: the model has no host duals")
        if self.has_shared:
            raise ValueError("dump: the model file format has no shared pairwise tables (expand_shared() gives a model it can hold)")
        if self.has_diff:
            raise ValueError("dump: the model file format has no difference-indexed pairwise factors (expand_diff() gives a model it can hold)")
        const = np.zeros(0) if self.const_data is None else np.ascontiguousarray(self.const_data, np.float64)
        mt = np.array([[t.left_ftype, t.right_ftype, t.schedule, t.n_left, t.n_right, t.kind, t.param, t.flags] for t in self.mtypes], np.int32).reshape(-1, 8)
        head = np.array([0x4C504D504D4F444C, self.n_ftypes, len(self.mtypes), self.tab_nleft.shape[0], self.tab_data.shape[0], self.n_factors,
                         self.n_messages, self.rel_fwd.shape[0], self.rel_bwd.shape[0], const.shape[0], self.dual_data.shape[0]], np.int64)
        with open(path, "wb") as f:
            f.write(head.tobytes()); f.write(np.float64(self.constant).tobytes())
            for a, dt in ((self.ftype_computes_primal, np.uint8), (mt, np.int32), (self.tab_off, np.int64), (self.tab_data, np.int32), (self.tab_nleft, np.int32),
                          (self.f_type, np.int32), (self.f_kind, np.uint8), (self.f_flags, np.uint8), (self.f_dim0, np.int32), (self.f_dim1, np.int32),
                          (const, np.float64), (self.dual_data, np.float64), (self.m_type, np.int32), (self.m_left, np.int32), (self.m_right, np.int32),
                          (self.rel_fwd, np.int32), (self.rel_bwd, np.int32)):
                f.write(np.ascontiguousarray(a, dt).tobytes())

    def c_struct(self) -> c_model:
        """ctypes view; arrays stay owned by ``self`` (borrowed for the duration of a call)."""
        mt = (c_msg_type * max(1, len(self.mtypes)))()
        for i, t in enumerate(self.mtypes):
            mt[i] = c_msg_type(t.left_ftype, t.right_ftype, t.schedule, t.n_left, t.n_right, t.kind, t.param, t.flags)
        self._keep = [mt]
        m = c_model()
        m.n_ftypes = self.n_ftypes
        m.ftype_computes_primal = _ptr(self.ftype_computes_primal)
        m.n_mtypes = len(self.mtypes)
        m.mtypes = C.addressof(mt)
        m.n_tables = int(self.tab_nleft.shape[0])
        m.tab_off, m.tab_data, m.tab_nleft = _ptr(self.tab_off), _ptr(self.tab_data), _ptr(self.tab_nleft)
        m.n_factors = self.n_factors
        m.f_type, m.f_kind, m.f_flags = _ptr(self.f_type), _ptr(self.f_kind), _ptr(self.f_flags)
        m.f_dim0, m.f_dim1 = _ptr(self.f_dim0), _ptr(self.f_dim1)
        m.const_data, m.dual_data = _ptr(self.const_data), _ptr(self.dual_data)
        m.n_messages = self.n_messages
        m.m_type, m.m_left, m.m_right = _ptr(self.m_type), _ptr(self.m_left), _ptr(self.m_right)
        m.n_rel_fwd, m.rel_fwd = int(self.rel_fwd.shape[0]), _ptr(self.rel_fwd)
        m.n_rel_bwd, m.rel_bwd = int(self.rel_bwd.shape[0]), _ptr(self.rel_bwd)
        m.constant = float(self.constant)
        if self.part_pairs is not None and len(self.part_pairs):
            self.part_pairs = np.ascontiguousarray(self.part_pairs, np.int32).reshape(-1, 2)
            m.n_part_pairs, m.part_pairs = int(self.part_pairs.shape[0]), _ptr(self.part_pairs)
        else:
            m.n_part_pairs, m.part_pairs = 0, None
        if self.n_shared_tables:
            self.sh_off = np.ascontiguousarray(self.sh_off, np.int64)
            self.sh_dim0 = np.ascontiguousarray(self.sh_dim0, np.int32)
            self.sh_dim1 = np.ascontiguousarray(self.sh_dim1, np.int32)
            self.sh_data = np.ascontiguousarray(self.sh_data, np.float64)
            m.n_shared_tables = self.n_shared_tables
            m.sh_off, m.sh_dim0, m.sh_dim1, m.sh_data = _ptr(self.sh_off), _ptr(self.sh_dim0), _ptr(self.sh_dim1), _ptr(self.sh_data)
        else:
            m.n_shared_tables, m.sh_off, m.sh_dim0, m.sh_dim1, m.sh_data = 0, None, None, None, None
        if self.f_table is not None:
            self.f_table = np.ascontiguousarray(self.f_table, np.int32)
        m.f_table = _ptr(self.f_table)
        return m


def refuse_shared(model: "FlatModel", who: str):
    """hosts that do not know the F_PAIRWISE_SHARED kind say so instead of misreading the model"""
    if model.has_shared:
        raise ValueError(who + " do not take models with shared pairwise tables (LPMP_F_PAIRWISE_SHARED): expand_shared() gives the "
                         "same model with one private dense table per factor")
    if model.has_diff:
        raise ValueError(who + " do not take models with difference-indexed pairwise factors (LPMP_F_PAIRWISE_DIFF): expand_diff() gives "
                         "the same model with one private dense table per factor")


def truncated_linear(d0: int, d1: int, slope: float, trunc: float) -> np.ndarray:
    """the difference vector D[k] = min(slope * |k - (d1 - 1)|, trunc) of a d0 x d1 DIFF factor: cost(a, b) = min(slope * |a - b|, trunc)
    (one multiply per entry: these host values are the values)"""
    k = np.abs(np.arange(d0 + d1 - 1, dtype=np.float64) - (d1 - 1))
    return np.minimum(np.float64(slope) * k, np.float64(trunc))


def diff_shift_int(shift) -> int:
    """the shift of a DIFF_SHIFT factor as the device converts the double (kernels.hip, diff_shift_int): NaN -> 0, saturated to
    [-2^30, 2^30], truncated toward zero.  A valid shift (ModelBuilder refuses anything else) is its own value."""
    x = float(shift)
    if x != x:
        return 0
    return int(min(max(x, -float(DIFF_SHIFT_MAX)), float(DIFF_SHIFT_MAX)))


def check_diff_shifts(shifts, who: str) -> np.ndarray:
    """``shifts`` as doubles; anything but integer values with |s| <= 2^30 is refused (the C ABI does not look at them)"""
    s = np.atleast_1d(np.asarray(shifts, np.float64))
    if not np.all(np.isfinite(s)) or np.any(s != np.trunc(s)) or np.any(np.abs(s) > DIFF_SHIFT_MAX):
        raise ValueError(who + ": a shift is an integer-valued number with |shift| <= 2^30")
    return s


def truncated_linear_compact(slope: float, trunc: float) -> tuple:
    """(D, zero_index): min(slope * |k|, trunc) for k = -T ... T with T the first difference at which the truncation holds —
    2 T + 1 entries whatever the label counts.  For DIFF_SHIFT factors: the clamped index continues D with its end values, which
    ARE the truncation, so the factor is the full-range potential exactly.  zero_index = T is where difference 0 sits
    (window_shift).  The entries are those of truncated_linear, to the bit."""
    slope, trunc = np.float64(slope), np.float64(trunc)
    if not (slope > 0 and trunc >= 0 and np.isfinite(slope) and np.isfinite(trunc)):
        raise ValueError("truncated_linear_compact: slope > 0 and trunc >= 0 are expected")
    T = 0
    while slope * np.float64(T) < trunc:
        T += 1
    k = np.abs(np.arange(-T, T + 1, dtype=np.float64))
    return np.minimum(slope * k, trunc), T


def truncated_quadratic_compact(slope: float, trunc: float) -> tuple:
    """the quadratic twin: min(slope * k^2, trunc) for k = -T ... T, the entries of truncated_quadratic to the bit"""
    slope, trunc = np.float64(slope), np.float64(trunc)
    if not (slope > 0 and trunc >= 0 and np.isfinite(slope) and np.isfinite(trunc)):
        raise ValueError("truncated_quadratic_compact: slope > 0 and trunc >= 0 are expected")
    T = 0
    while slope * (np.float64(T) * np.float64(T)) < trunc:
        T += 1
    k = np.arange(-T, T + 1, dtype=np.float64)
    return np.minimum(slope * (k * k), trunc), T


def window_shift(c_left, c_right, zero_index):
    """the shift of a DIFF_SHIFT factor between a variable that holds the absolute labels c_left, c_left + 1, ... (side 0) and
    one that holds c_right, ... (side 1), for a vector whose entry ``zero_index`` is difference 0: label pair (a, b) stands for
    the difference (a + c_left) - (b + c_right), which is entry a - b + shift.  Arrays give one shift per factor."""
    return np.asarray(c_left, np.int64) - np.asarray(c_right, np.int64) + np.int64(zero_index)


MOVE_DELTA_MAX = 1 << 20      # |delta| of a window move (include/lpmp_engine.h, lpmp_move_windows)
MOVE_MAX_LABELS = 512         # a listed unary's label count


class WindowsUnsupported(ValueError):
    """``window_links`` / ``move_windows``: a listed factor the move does not take (lpmp_window_set_create: LPMP_ERR_UNSUPPORTED)"""

    def __init__(self, factor: int, msg: str):
        super().__init__(msg)
        self.factor = factor


def window_links(model: "FlatModel", factors=None):
    """(factors, links, pairs) of a window set, by the rules of lpmp_window_set_create: ``factors`` as an int array (None: every
    VECTOR factor), ``links[i]`` = [(pairwise factor, side)] of listed factor i, ``pairs`` = [(DIFF_SHIFT factor, row of the listed
    unary on side 0 or -1, ... on side 1)] in the order the listed unaries meet them.  ValueError for an index out of range, a
    non-VECTOR factor or a factor listed twice; WindowsUnsupported naming the lowest listed factor the move does not take."""
    nf = model.n_factors
    if factors is None:
        factors = np.flatnonzero(model.f_kind == F_VECTOR)
    factors = np.asarray(factors, np.int64).reshape(-1)
    row_of = {}
    for i, f in enumerate(factors):
        f = int(f)
        if f < 0 or f >= nf:
            raise ValueError(f"window set: factor index {f} (entry {i}) is out of range")
        if model.f_kind[f] != F_VECTOR:
            raise ValueError(f"window set: factor {f} (entry {i}) is not a VECTOR factor")
        if f in row_of:
            raise ValueError(f"window set: factor {f} (entry {i}) is listed twice")
        row_of[f] = i
    of_factor = {}                       # factor -> [(message, role)] in message order
    for k in range(model.n_messages):
        of_factor.setdefault(int(model.m_left[k]), []).append((k, 0))
        of_factor.setdefault(int(model.m_right[k]), []).append((k, 1))
    bad = {}

    def refuse(u, what):
        bad.setdefault(u, f"window set: factor {u} {what}")

    def side_unaries(p):
        out = [-1, -1]
        for k, role in of_factor.get(p, []):
            t = model.mtypes[int(model.m_type[k])]
            if role != 1 or t.kind != M_UNARY_PAIRWISE or t.param not in (0, 1):
                continue
            u = int(model.m_left[k])
            out[t.param] = u if out[t.param] in (-1, u) else -2
        return out
    links, pairs, pair_of = [], [], {}
    for f in factors:
        u = int(f)
        d = int(model.f_dim0[u])
        mine = []
        if d > MOVE_MAX_LABELS:
            refuse(u, f"has {d} labels (at most {MOVE_MAX_LABELS})")
        for k, role in of_factor.get(u, []):
            t = model.mtypes[int(model.m_type[k])]
            p = int(model.m_right[k])
            if role != 0 or t.kind != M_UNARY_PAIRWISE or model.f_kind[p] != F_PAIRWISE_DIFF_SHIFT or t.param not in (0, 1):
                refuse(u, "has a message that is not a unary-pairwise message with the factor as its unary and a DIFF_SHIFT factor on the right")
                continue
            if int(model.f_dim1[p] if t.param else model.f_dim0[p]) != d:
                refuse(u, f"and side {t.param} of factor {p} differ in their label counts")
                continue
            if (p, t.param) in mine:
                refuse(u, f"has two messages into one vector of factor {p}")
                continue
            mine.append((p, t.param))
            if p not in pair_of:
                su = side_unaries(p)
                pair_of[p] = -2 if -2 in su else len(pairs)
                if pair_of[p] >= 0:
                    pairs.append((p, row_of.get(su[0], -1), row_of.get(su[1], -1)))
            if pair_of[p] == -2:
                refuse(u, f"is next to DIFF_SHIFT factor {p}, which has two different unaries on one side")
        links.append(mine)
    if bad:
        u = min(bad)
        raise WindowsUnsupported(u, bad[u])
    return factors, links, pairs


def move_windows(model: "FlatModel", duals, factors, delta, cost_old=None, cost_new=None):
    """The numpy statement of lpmp_move_windows (include/lpmp_engine.h has the rule): the windows of the listed VECTOR ``factors``
    (None: all of them) move by ``delta[i]`` labels.  Returns ``(model', duals')``: a model with a new const array holding the new
    shifts (every other array shared with ``model``), and the moved packed duals —
    theta_u'[x] = theta_u[g(x)] and m_{p,s}'[x] = m_{p,s}[g(x)] with g(x) = clip(x + delta_u, 0, d_u - 1) for every listed u and each
    of its messages; shift' = clip(diff_shift_int(shift) + delta_l - delta_r, -2^30, 2^30) for every adjacent DIFF_SHIFT factor whose
    two deltas differ; with ``cost_old`` / ``cost_new`` ([n, >= longest vector], both or neither) theta_u'[x] = theta_u[g] +
    (cost_new[i][x] - cost_old[i][g]) wherever the two cost entries do not compare equal.  The yardstick of the device call."""
    import dataclasses
    factors, links, pairs = window_links(model, factors)
    n = factors.shape[0]
    delta = np.asarray(delta).reshape(-1)
    if delta.shape[0] != n or (n and not np.issubdtype(delta.dtype, np.integer)):
        raise ValueError("move_windows: one integer delta per listed factor")
    delta = delta.astype(np.int64)
    if np.any(np.abs(delta) > MOVE_DELTA_MAX):
        raise ValueError("move_windows: |delta| <= 2^20")
    if (cost_old is None) != (cost_new is None):
        raise ValueError("move_windows: cost_old and cost_new come together, or not at all")
    if model.const_data is None:
        raise ValueError("move_windows: the model has no host constants")
    doff, coff = model.dual_offsets(), model.const_offsets()
    out = np.array(duals, np.float64, copy=True)
    src = np.asarray(duals, np.float64)
    if src.shape != (int(doff[-1]),):
        raise ValueError("move_windows: duals packed as FlatModel.dual_data are expected")
    const = np.array(model.const_data, np.float64, copy=True)
    if cost_old is not None:
        cost_old, cost_new = np.asarray(cost_old, np.float64), np.asarray(cost_new, np.float64)
    for i, u in enumerate(factors):
        u = int(u)
        d = int(model.f_dim0[u])
        g = np.clip(np.arange(d, dtype=np.int64) + delta[i], 0, d - 1)
        th = src[doff[u]: doff[u] + d][g]
        if cost_old is not None:
            cn, co = cost_new[i, :d], cost_old[i, :d][g]
            with np.errstate(invalid="ignore"):
                th = np.where(cn == co, th, th + (cn - co))
        out[doff[u]: doff[u] + d] = th
        for p, side in links[i]:
            at = int(doff[p]) + (int(model.f_dim0[p]) if side else 0)
            out[at: at + d] = src[at: at + d][g]
    for p, lrow, rrow in pairs:
        dl = int(delta[lrow]) if lrow >= 0 else 0
        dr = int(delta[rrow]) if rrow >= 0 else 0
        if dl != dr:
            s = diff_shift_int(const[coff[p] + 1]) + dl - dr
            const[coff[p] + 1] = np.float64(min(max(s, -DIFF_SHIFT_MAX), DIFF_SHIFT_MAX))
    return dataclasses.replace(model, const_data=const, _keep=[]), out


def move_labels(primal, model: "FlatModel", factors, delta):
    """The numpy statement of what lpmp_move_windows_carry does to the labels (include/lpmp_engine.h has the rule).  ``primal`` is the
    [n_factors, 2] array of ``Engine.download_primal``; the windows of the listed VECTOR ``factors`` (None: all of them) move by
    ``delta[i]`` labels, a delta beyond +-2^20 saturated as the device saturates it.  Returns a new array: a listed unary with a label
    x < d gets min(max(x - delta_i, 0), d - 1) — new label x is old label x + delta, so what named old x names x - delta —, an unset
    entry (the dimension) stays unset, unlisted unaries keep their labels, and then side s of every pairwise factor takes the label
    of its unary over every unary-pairwise message whose unary holds one, as after a decode.  On a model the rounding code refuses
    (a message type that is not unary-pairwise) no pairwise slot is written."""
    out = np.array(primal, np.int32, copy=True)
    if out.shape != (model.n_factors, 2):
        raise ValueError("move_labels: a [n_factors, 2] primal array is expected")
    if factors is None:
        factors = np.flatnonzero(model.f_kind == F_VECTOR)
    factors = np.asarray(factors, np.int64).reshape(-1)
    delta = np.asarray(delta).reshape(-1)
    if delta.shape[0] != factors.shape[0] or (factors.shape[0] and not np.issubdtype(delta.dtype, np.integer)):
        raise ValueError("move_labels: one integer delta per listed factor")
    delta = np.clip(delta.astype(np.int64), -MOVE_DELTA_MAX, MOVE_DELTA_MAX)
    for i, u in enumerate(factors):
        u = int(u)
        d, x = int(model.f_dim0[u]), int(out[u, 0])
        if 0 <= x < d:
            out[u, 0] = min(max(x - int(delta[i]), 0), d - 1)
    if all(t.kind == M_UNARY_PAIRWISE for t in model.mtypes):
        for k in range(model.n_messages):
            u, p = int(model.m_left[k]), int(model.m_right[k])
            if out[u, 0] < model.f_dim0[u]:
                out[p, int(model.mtypes[int(model.m_type[k])].param)] = out[u, 0]
    return out


def truncated_quadratic(d0: int, d1: int, slope: float, trunc: float) -> np.ndarray:
    """D[k] = min(slope * (k - (d1 - 1))^2, trunc): the square is exact in double, then one multiply"""
    k = np.arange(d0 + d1 - 1, dtype=np.float64) - (d1 - 1)
    return np.minimum(np.float64(slope) * (k * k), np.float64(trunc))


DIFF_BAND_DIV = 4      # plan.hpp: a band of at most n / DIFF_BAND_DIV entries runs the banded kernel


def diff_band(D) -> tuple:
    """the band (lo, hi) of a difference vector, as the planner detects it (plan.cpp, diff_band): every entry below lo has the
    BITS of D[0], every entry above hi the bits of D[n - 1] (-0.0 and +0.0 differ).  lo = the first index whose entry is not D[0]
    (n if none), hi = the last index >= lo whose entry is not D[n - 1] (lo - 1 if none); hi - lo + 1 >= 0 is the width"""
    b = np.ascontiguousarray(D, np.float64).reshape(-1).view(np.uint64)
    n = b.shape[0]
    left = np.flatnonzero(b != b[0])
    lo = int(left[0]) if left.size else n
    right = np.flatnonzero(b[lo:] != b[n - 1])
    hi = lo + int(right[-1]) if right.size else lo - 1
    return lo, hi


def diff_band_is_banded(D) -> bool:
    """the rule of the banded kernel: the band has at most n / DIFF_BAND_DIV entries"""
    lo, hi = diff_band(D)
    return (hi - lo + 1) * DIFF_BAND_DIV <= np.asarray(D).size


def diff_shift_band(D, d0: int, d1: int, shift) -> tuple:
    """the band (le, he) of a DIFF_SHIFT receive: of the expansion D[clip(i - off, 0, n - 1)], i = a - b + d1 - 1 in [0, d0 + d1 - 1),
    off = d1 - 1 - diff_shift_int(shift).  The band (lo, hi) of D moved by off and clipped to the expansion: every entry below le is
    D[0], every entry above he is D[n - 1], entry i in [le, he] is D[i - off]; he >= le - 1.  (kernels.hip, sweep_diff_shift_band_kernel.)
    Where an end of the expansion falls inside the band, le / he is that end and not the first / last entry that differs from it:
    a bound of the band, which is all the reduction needs"""
    lo, hi = diff_band(D)
    ne = d0 + d1 - 1
    off = d1 - 1 - diff_shift_int(shift)
    return min(max(lo + off, 0), ne), min(max(hi + off, -1), ne - 1)


def diff_shift_is_banded(D, d0: int, d1: int) -> bool:
    """the rule of the shifted banded kernel for a d0 x d1 receive: the band of D itself has at most (d0 + d1 - 1) / DIFF_BAND_DIV
    entries.  The shift moves the band and never widens it: it is not an argument"""
    lo, hi = diff_band(D)
    return (hi - lo + 1) * DIFF_BAND_DIV <= d0 + d1 - 1


def forests_from_paths(path_groups):
    """the groups of ``Engine.path_set`` (a sequence of groups, each a sequence of paths of factor indices) as the forest groups of
    ``Engine.forest_set``: one (unaries, parent) int32 array pair per group, the parent of a member the NEXT member of its path
    and the last member the root — the rooting under which a forest move gives the labels of the path move bit for bit"""
    out = []
    for g in path_groups:
        un = [int(f) for path in g for f in path]
        par = [int(q) for path in g for q in list(path[1:]) + [-1]]
        out.append((np.asarray(un, np.int32).reshape(-1), np.asarray(par, np.int32).reshape(-1)))
    return out


class ModelBuilder:
    """Collects factors / messages / relations in insertion order (bulk or one at a time)."""

    def __init__(self, n_ftypes: int, mtypes: Sequence[MsgType], ftype_computes_primal: Optional[Sequence[int]] = None):
        self.n_ftypes = int(n_ftypes)
        self.mtypes = list(mtypes)
        self.ftype_computes_primal = np.zeros(self.n_ftypes, np.uint8) if ftype_computes_primal is None \
            else np.asarray(ftype_computes_primal, np.uint8)
        self._tables: List[np.ndarray] = []
        self._tab_nleft: List[int] = []
        self._shared: List[np.ndarray] = []     # shared pairwise tables, [d0, d1] each
        self._f_table = []                       # (first factor id, table ids) of every add_shared_pairwise call
        self._f = []      # (type, kind, flags, dim0, dim1) array chunks
        self._const = []
        self._dual = []
        self._nf = 0
        self._m = []
        self._nm = 0
        self._rel_fwd = []
        self._rel_bwd = []
        self._part = []
        self.constant = 0.0
        self.skip_const = False  # True: const tables live only on the device (see Engine.upload)
        self.skip_dual = False   # True: so do the duals (upload(dual_dev=...)): no host copy of them is built

    # -- labeling match tables (reference labeling_list_factor.hxx:384-402) ------------------
    def add_labeling_table(self, left_labelings, right_labelings, indices) -> int:
        """``labeling_message<LEFT, RIGHT, INDICES...>``: table[r] = index of the left labeling whose
        labels equal the right labeling's labels at ``indices``, or n_left if none."""
        left = [tuple(l) for l in left_labelings]
        tab = []
        for r in right_labelings:
            sub = tuple(r[i] for i in indices)
            tab.append(left.index(sub) if sub in left else len(left))
        self._tables.append(np.asarray(tab, np.int32))
        self._tab_nleft.append(len(left))
        return len(self._tables) - 1

    # -- factors ---------------------------------------------------------------------------------
    def _add_factors(self, n, ftype, kind, flags, dim0, dim1, const, dual):
        ids = np.arange(self._nf, self._nf + n, dtype=np.int32)
        self._f.append((np.full(n, ftype, np.int32), np.full(n, kind, np.uint8), np.full(n, flags, np.uint8),
                        np.full(n, dim0, np.int32), np.full(n, dim1, np.int32)))
        if const is not None:
            self._const.append(np.ascontiguousarray(const, np.float64).reshape(-1))
        if not self.skip_dual:
            self._dual.append(np.ascontiguousarray(dual, np.float64).reshape(-1))
        self._nf += n
        return ids

    def add_vector_factors(self, ftype: int, costs, implicit_origin: bool = False, shape=None) -> np.ndarray:
        """UnarySimplexFactor / labeling_factor / test_factor; ``costs`` is [n, dim] (None with skip_dual: ``shape`` = (n, dim))."""
        if costs is None:
            assert self.skip_dual and shape is not None
            n, dim = shape
        else:
            costs = np.atleast_2d(np.asarray(costs, np.float64))
            n, dim = costs.shape
        return self._add_factors(n, ftype, F_VECTOR, FF_IMPLICIT_ORIGIN if implicit_origin else 0, dim, 0, None, costs)

    def add_dense_pairwise(self, ftype: int, tables=None, n: Optional[int] = None, dims=None) -> np.ndarray:
        """PairwiseSimplexFactor; ``tables`` is [n, d0, d1] (row-major) or None with skip_const."""
        if tables is not None:
            tables = np.asarray(tables, np.float64)
            if tables.ndim == 2:
                tables = tables[None]
            n, d0, d1 = tables.shape
        else:
            assert self.skip_const and n is not None and dims is not None
            d0, d1 = dims
        return self._add_factors(n, ftype, F_PAIRWISE_DENSE, 0, d0, d1, tables, None if self.skip_dual else np.zeros((n, d0 + d1)))

    def add_potts_pairwise(self, ftype: int, n_labels: int, diffs) -> np.ndarray:
        """pairwise_potts_factor(n_labels, diff)."""
        diffs = np.atleast_1d(np.asarray(diffs, np.float64))
        n = diffs.shape[0]
        return self._add_factors(n, ftype, F_PAIRWISE_POTTS, 0, n_labels, n_labels, diffs, None if self.skip_dual else np.zeros((n, 2 * n_labels)))

    def add_shared_table(self, table) -> int:
        """a pairwise table V [d0, d1] that any number of factors may use (add_shared_pairwise); returns its id"""
        table = np.ascontiguousarray(table, np.float64)
        if table.ndim != 2 or table.shape[0] < 1 or table.shape[1] < 1:
            raise ValueError("add_shared_table: a [d0, d1] table is expected")
        self._shared.append(table.copy())
        return len(self._shared) - 1

    def add_shared_pairwise(self, ftype: int, table_ids, scales) -> np.ndarray:
        """pairwise factors cost(a, b) = scales[i] * V[table_ids[i]][a][b]: every factor holds one double.  All tables of one
        call must have the same dims (factors of other dims: another call).  ``scales`` is finite, and positive where the
        table holds +inf entries."""
        table_ids = np.atleast_1d(np.asarray(table_ids, np.int32))
        scales = np.atleast_1d(np.asarray(scales, np.float64))
        if scales.shape[0] == 1 and table_ids.shape[0] > 1:
            scales = np.full(table_ids.shape[0], scales[0])
        if table_ids.shape != scales.shape or table_ids.shape[0] == 0:
            raise ValueError("add_shared_pairwise: one table id and one scale per factor")
        if table_ids.min() < 0 or table_ids.max() >= len(self._shared):
            raise ValueError("add_shared_pairwise: table id out of range")
        dims = {self._shared[t].shape for t in np.unique(table_ids)}
        if len(dims) != 1:
            raise ValueError("add_shared_pairwise: the tables of one call must have the same dims")
        d0, d1 = dims.pop()
        n = table_ids.shape[0]
        ids = self._add_factors(n, ftype, F_PAIRWISE_SHARED, 0, d0, d1, scales, None if self.skip_dual else np.zeros((n, d0 + d1)))
        self._f_table.append((int(ids[0]), table_ids.copy()))
        return ids

    def add_diff_table(self, vec) -> int:
        """a difference vector D, stored as a [1, n] entry of the shared pool; returns its id.  Any length n >= 1: add_diff_pairwise
        (cost(a, b) = scale * D[a - b + d1 - 1]) takes the vectors of d0 + d1 - 1 entries, add_diff_shift_pairwise any"""
        vec = np.ascontiguousarray(vec, np.float64)
        if vec.ndim != 1 or vec.shape[0] < 1:
            raise ValueError("add_diff_table: a vector is expected")
        self._shared.append(vec.reshape(1, -1).copy())
        return len(self._shared) - 1

    def add_diff_pairwise(self, ftype: int, d0: int, d1: int, table_ids, scales) -> np.ndarray:
        """d0 x d1 pairwise factors cost(a, b) = scales[i] * D[table_ids[i]][a - b + d1 - 1]: every factor holds one double.
        ``scales`` is finite, and positive where the vector holds +inf entries."""
        table_ids = np.atleast_1d(np.asarray(table_ids, np.int32))
        scales = np.atleast_1d(np.asarray(scales, np.float64))
        if scales.shape[0] == 1 and table_ids.shape[0] > 1:
            scales = np.full(table_ids.shape[0], scales[0])
        if table_ids.shape != scales.shape or table_ids.shape[0] == 0:
            raise ValueError("add_diff_pairwise: one table id and one scale per factor")
        if table_ids.min() < 0 or table_ids.max() >= len(self._shared):
            raise ValueError("add_diff_pairwise: table id out of range")
        d0, d1 = int(d0), int(d1)
        if d0 < 1 or d1 < 1 or any(self._shared[t].shape != (1, d0 + d1 - 1) for t in np.unique(table_ids)):
            raise ValueError("add_diff_pairwise: a %d x %d factor needs difference vectors of %d entries" % (d0, d1, d0 + d1 - 1))
        n = table_ids.shape[0]
        ids = self._add_factors(n, ftype, F_PAIRWISE_DIFF, 0, d0, d1, scales, None if self.skip_dual else np.zeros((n, d0 + d1)))
        self._f_table.append((int(ids[0]), table_ids.copy()))
        return ids

    def add_diff_shift_pairwise(self, ftype: int, d0: int, d1: int, table_ids, scales, shifts) -> np.ndarray:
        """d0 x d1 pairwise factors cost(a, b) = scales[i] * D[clip(a - b + shifts[i], 0, n - 1)] with D = vector table_ids[i] of
        ANY length n: every factor holds two doubles {scale, shift}.  ``scales`` as for add_diff_pairwise; ``shifts`` are integers
        with |shift| <= 2^30 (window_shift gives the one of two label windows)."""
        table_ids = np.atleast_1d(np.asarray(table_ids, np.int32))
        n = table_ids.shape[0]
        scales = np.atleast_1d(np.asarray(scales, np.float64))
        shifts = check_diff_shifts(shifts, "add_diff_shift_pairwise")
        if scales.shape[0] == 1 and n > 1:
            scales = np.full(n, scales[0])
        if shifts.shape[0] == 1 and n > 1:
            shifts = np.full(n, shifts[0])
        if table_ids.shape != scales.shape or table_ids.shape != shifts.shape or n == 0:
            raise ValueError("add_diff_shift_pairwise: one table id, one scale and one shift per factor")
        if table_ids.min() < 0 or table_ids.max() >= len(self._shared):
            raise ValueError("add_diff_shift_pairwise: table id out of range")
        d0, d1 = int(d0), int(d1)
        if d0 < 1 or d1 < 1 or any(self._shared[t].shape[0] != 1 for t in np.unique(table_ids)):
            raise ValueError("add_diff_shift_pairwise: positive dims and difference VECTORS (add_diff_table) are expected")
        ids = self._add_factors(n, ftype, F_PAIRWISE_DIFF_SHIFT, 0, d0, d1, np.stack([scales, shifts], 1), None if self.skip_dual else np.zeros((n, d0 + d1)))
        self._f_table.append((int(ids[0]), table_ids.copy()))
        return ids

    # -- messages / relations ------------------------------------------------------------------------
    def add_messages(self, mtype: int, left, right) -> np.ndarray:
        left = np.atleast_1d(np.asarray(left, np.int32))
        right = np.atleast_1d(np.asarray(right, np.int32))
        assert left.shape == right.shape
        n = left.shape[0]
        ids = np.arange(self._nm, self._nm + n, dtype=np.int64)
        self._m.append((np.full(n, mtype, np.int32), left, right))
        self._nm += n
        return ids

    def add_interleaved_messages(self, mtypes, left, right, return_ids: bool = True):
        """Messages of several types in one insertion sequence (row i has type mtypes[i])."""
        mtypes = np.asarray(mtypes, np.int32)
        left = np.asarray(left, np.int32)
        right = np.asarray(right, np.int32)
        n = left.shape[0]
        ids = np.arange(self._nm, self._nm + n, dtype=np.int64) if return_ids else None
        self._m.append((mtypes, left, right))
        self._nm += n
        return ids

    def add_relations(self, f1, f2):
        """AddFactorRelation(f1, f2): f1 before f2 forward, f2 before f1 backward."""
        f1 = np.atleast_1d(np.asarray(f1, np.int32))
        f2 = np.atleast_1d(np.asarray(f2, np.int32))
        fwd = np.empty((f1.shape[0], 2), np.int32); fwd[:, 0] = f1; fwd[:, 1] = f2
        bwd = np.empty((f1.shape[0], 2), np.int32); bwd[:, 0] = f2; bwd[:, 1] = f1
        self._rel_fwd.append(fwd)
        self._rel_bwd.append(bwd)

    def put_in_same_partition(self, f1, f2):
        """LP::put_in_same_partition(f1, f2) (reference LP_MP.h:465)"""
        self._part.append(np.stack([np.atleast_1d(np.asarray(f1, np.int32)), np.atleast_1d(np.asarray(f2, np.int32))], 1))

    def add_forward_relations(self, f1, f2):
        self._rel_fwd.append(np.stack([np.atleast_1d(np.asarray(f1, np.int32)), np.atleast_1d(np.asarray(f2, np.int32))], 1))

    def add_backward_relations(self, f1, f2):
        self._rel_bwd.append(np.stack([np.atleast_1d(np.asarray(f1, np.int32)), np.atleast_1d(np.asarray(f2, np.int32))], 1))

    def finish(self) -> FlatModel:
        def cat(chunks, dtype, shape=(0,)):
            if len(chunks) == 1:                       # (models of millions of factors: no second copy of a single block)
                return np.ascontiguousarray(chunks[0])
            return np.ascontiguousarray(np.concatenate(chunks)) if chunks else np.zeros(shape, dtype)
        tab_off = np.concatenate([[0], np.cumsum([len(t) for t in self._tables])]).astype(np.int64)
        shared = {}
        if self._shared:
            shared = dict(sh_off=np.concatenate([[0], np.cumsum([t.size for t in self._shared])]).astype(np.int64),
                          sh_dim0=np.asarray([t.shape[0] for t in self._shared], np.int32),
                          sh_dim1=np.asarray([t.shape[1] for t in self._shared], np.int32),
                          sh_data=np.ascontiguousarray(np.concatenate([t.reshape(-1) for t in self._shared])))
        if self._f_table:
            f_table = np.full(self._nf, -1, np.int32)
            for first, t in self._f_table:
                f_table[first: first + t.shape[0]] = t
            shared["f_table"] = f_table
        return FlatModel(
            **shared,
            n_ftypes=self.n_ftypes, ftype_computes_primal=self.ftype_computes_primal, mtypes=self.mtypes,
            tab_off=tab_off, tab_data=cat(self._tables, np.int32), tab_nleft=np.asarray(self._tab_nleft, np.int32),
            f_type=cat([c[0] for c in self._f], np.int32), f_kind=cat([c[1] for c in self._f], np.uint8),
            f_flags=cat([c[2] for c in self._f], np.uint8), f_dim0=cat([c[3] for c in self._f], np.int32),
            f_dim1=cat([c[4] for c in self._f], np.int32),
            const_data=None if self.skip_const else cat(self._const, np.float64),
            dual_data=None if self.skip_dual else cat(self._dual, np.float64),
            m_type=cat([c[0] for c in self._m], np.int32), m_left=cat([c[1] for c in self._m], np.int32),
            m_right=cat([c[2] for c in self._m], np.int32),
            rel_fwd=cat(self._rel_fwd, np.int32, (0, 2)).astype(np.int32, copy=False).reshape(-1, 2),
            rel_bwd=cat(self._rel_bwd, np.int32, (0, 2)).astype(np.int32, copy=False).reshape(-1, 2),
            constant=self.constant,
            part_pairs=cat(self._part, np.int32, (0, 2)).astype(np.int32).reshape(-1, 2) if self._part else None)
