"""Session tests: random call sequences on ONE engine against the oracle (tests/test_session_host.py, tests/test_session_gpu.py,
tests/session_replay.py).  The engine keeps much derived state between calls (tracked bounds, the rows layout and its two flags,
speculative batches, the cache of joined-pass chains, labels and their time stamp, decode tables, read-outs, prepared schedules,
``const_bad``, the float tables, the pool cells); every call has to leave all of it right for every call that may follow.  A session
is a list of ``(op, args)`` steps — a pure function of (cell, seed, n) — applied to an engine and to a ``Shadow`` that states
every call in numpy / on the CPU oracle; everything the caller can observe is compared.

The contract, call by call (op -> paragraph of include/lpmp_engine.h -> statement the shadow uses).  "rebuild" = a new ``Oracle`` on
``oracle_model(with_duals(model, duals))`` with send rule and weight mode set again; "labels unset" = every slot holds its dimension.

  op                          header paragraph                          statement
  --------------------------  ----------------------------------------  ------------------------------------------------------------
  upload                      lpmp_upload_model, lpmp_set_rows_layout,  new model, its duals, no weight mode, labels unset, every
                              lpmp_set_table_precision                  schedule id and read-out of the old model dead; the send rule
                                                                        stays.  f32 tables + rows layout: LPMP_ERR_UNSUPPORTED and
                                                                        NO model afterwards (every call LPMP_ERR_STATE)
  compute_pass(n)             lpmp_compute_pass                         Oracle.ComputePass(n)
  forward_ / backward_pass    lpmp_compute_forward_ / _backward_pass    Oracle.ComputeForwardPass / ComputeBackwardPass
  compute_pass_custom         lpmp_compute_pass_custom                  Oracle.compute_pass_custom(test_fuzz_gpu.random_rows)
  schedule_create / run       lpmp_schedule_create_fused / _run         the rows are kept; run = Oracle.compute_pass_custom(rows)
  schedule_destroy            lpmp_schedule_destroy, lpmp_schedule_run  the id is dead: LPMP_ERR_INVALID from then on
  ..._pass_and_primal(it)     primal rounding inside the sweep          Oracle.Compute...PassAndPrimal(it); labels = Oracle.primal()
  decode_primal(d, refine)    lpmp_decode_primal                        labels = decode_cases.decode_reference; duals do not move
  set_reparametrization       lpmp_set_reparametrization                Oracle.set_reparametrization
  set_reparametrization_type  lpmp_set_reparametrization_type           Oracle.set_reparametrization_type (SHARED / RESIDUAL)
  knobs                       lpmp_set_speculation ("results never      nothing: set_speculation, set_persistent_launches,
                              differ"), lpmp_set_persistent_launches    enable_ / reset_kernel_timing, prepare_passes,
                              ("same results"), lpmp_prepare_passes,    invalidate_lower_bounds, synchronize move no value
                              lpmp_invalidate_lower_bounds, ...
  upload_costs(const, duals)  lpmp_upload_costs, "duals given"          recost_cases.recost: model and duals replaced; labels unset
  upload_costs(const)         lpmp_upload_costs, "duals NOT given"      constants replaced, duals kept, labels unset
  set_vectors(new - old)      lpmp_zero_pairwise_duals (last sentence)  after every other warm start, as a step of its own:
                                                                        scatter_rows(all unaries, new - old, accumulate)
  set_vectors                 lpmp_set_vectors                          recost_cases.scatter_rows; labels stay
  zero_pairwise_duals         lpmp_zero_pairwise_duals                  recost_cases.zero_pairwise; labels stay
  set_constants               lpmp_set_constants                        repool_cases.with_rows; labels unset
  upload_shared_pool          lpmp_upload_shared_pool                   FlatModel.with_pool; duals kept; labels unset
  upload_duals                lpmp_upload_duals                         the duals given; labels stay
  window_set_create / destroy lpmp_window_set_create / _destroy         the list is kept by slot (None: every unary); create counts
                              ("counted ONCE by lpmp_schedules_built")  once in schedules_built; after an upload a move on it is
                                                                        LPMP_ERR_STATE and destroying it stays legal
  move_windows(form)          lpmp_move_windows ("moving label          lp_mp_amd.model.move_windows on the model and the duals: duals
                              windows"): delta / costs from the host    gathered, shifts of the adjacent DIFF_SHIFT factors replaced,
                              or from device memory, one delta for      labels unset, schedules_built unmoved; every schedule id and
                              all, all 0                                read-out stays.  The costs: the session's unaries (``nominal``)
                                                                        in the old window, move_windows_cases.cost_pair in the new
  (DIFF_SHIFT models)         lpmp_model.h, LPMP_F_PAIRWISE_DIFF_SHIFT  passes and bounds on ``expand_diff()``; decode, energy and
                                                                        beliefs on scale * D[clip(a - b + int(shift), 0, n - 1)]
                                                                        (decode_cases.cost_line, readout_cases.cost_table); new costs
                                                                        and listed rows give {scale, integer shift}
                                                                        (recost_cases.recost_shift, repool_cases.rows_for_shift)
  path_set_create / _destroy  lpmp_path_set_create ("counted ONCE by    the groups are kept by slot (path_list); create counts once in
                              lpmp_schedules_built")                    schedules_built; after an upload a move on the set is
                                                                        LPMP_ERR_STATE and destroying it stays legal
  forest_set_create/_destroy  lpmp_forest_set_create                    as above (forest_list; None: the cover of Plan.suggest_forests())
  path_moves(slot, rounds)    lpmp_path_moves / lpmp_forest_moves       labels = path_moves_cases.path_moves_reference /
  forest_moves(slot, rounds)  ("reads the duals, the constants and the  forest_moves_cases.forest_moves_reference(eff model, shadow
                              primal array, writes only the primal      duals, labels, groups, rounds), rounds in 0 .. 3.  Duals,
                              array")                                   bounds, weight mode, schedules, schedules_built, read-outs and
                                                                        window sets do not move
  upload_primal(seed, form)   lpmp_upload_primal                        the labels given (primal_for): random; partly_unset (some
                                                                        unaries hold their dimension); stray (negative entries).  A move
                                                                        counts an off-path neighbour's unset label as its last label and
                                                                        a negative one as 0 (the two ..._unset_neighbour_is_clamped tests)
  (a model the rounding code  the "array of unset labels" sentences of  the moves are stated on the grid that is the first factors of the
  refuses: rlists)            lpmp_path_moves / lpmp_forest_moves /     model, with the prefix of the duals and constants (move_model);
                              lpmp_readout_labels                       they write the unary slots only and no pairwise slot; ro_labels
                                                                        sees them; every cost change unsets them; a refused call
                                                                        (download_primal, evaluate_primal, check_primal_consistency,
                                                                        upload_primal, ..._pass_and_primal, decode_primal) leaves them
  lower_bound                 lpmp_lower_bound                          Oracle.LowerBound
  factor_lower_bounds         lpmp_factor_lower_bounds                  Oracle.factor_lower_bound per factor
  download_duals              lpmp_download_duals                       Oracle.duals
  labels                      lpmp_download_primal,                     the label array; consistent = every message's pairwise slot
                              lpmp_check_primal_consistency,            equals its unary's; cost = decode_cases.energy on the
                              lpmp_evaluate_primal                      original unaries theta_u + sum m_s (+inf: inconsistent / unset)
  read-out labels / vectors   lpmp_readout_labels / _vectors            the label column / readout_cases.vectors_np
  read-out beliefs            lpmp_readout_beliefs                      readout_cases.beliefs_np (floats widened under f32 tables)
  refused                     the refusal sentence of each call         the documented code, and nothing moves

Nothing an engine returns ever enters the shadow."""
import collections
import dataclasses
import functools
import zlib

import numpy as np

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import decode_cases as DC
import diff_shift_cases as DS
import forest_moves_cases as FM
import mixed_precision_cases as MP
import move_windows_cases as MW
import path_moves_cases as PM
import readout_cases as RO
import recost_cases as RC
import repool_cases as RP
from test_fuzz_gpu import random_rows

ERR_INVALID, ERR_UNSUPPORTED, ERR_DEVICE, ERR_STATE = -1, -2, -3, -4
ANISO = M.REPAM_ANISOTROPIC
MODES = (M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2, M.REPAM_UNIFORM, M.REPAM_DAMPED_UNIFORM)
RT_SHARED, RT_RESIDUAL = 0, 1
LB_RTOL = 1e-9            # tests/test_fuzz_gpu.py; a tracked and a recomputed sum differ in association (tests/test_bound_sum_gpu.py)
FLB_ATOL = 1e-12          # tests/test_fuzz_gpu.py, tests/test_recost_gpu.py on costs of this magnitude
ENERGY_RTOL = 1e-9        # tests/test_decode_gpu.py test_decoded_labels_are_consistent_and_cost_the_original_energy
PAIR_TOL = 1e-12          # tests/test_speculation_gpu.py lines 115-121: bounds of two engines, rtol = atol

OBSERVING = ("lb", "flb", "dl", "labels", "ro_labels", "ro_vectors", "ro_beliefs")
COST = ("cold", "warm", "vectors", "zero", "consts", "pool", "duals", "move")
STATE = ("pass", "dir", "custom", "primal_pass", "decode", "mode", "rtype", "knob") + COST + ("reupload", "refused", "relabel", "sets")
OP_CLASS = {
    "compute_pass": "pass", "forward_pass": "dir", "backward_pass": "dir",
    "compute_pass_custom": "custom", "schedule_create": "custom", "schedule_run": "custom", "schedule_destroy": "custom",
    "forward_pass_and_primal": "primal_pass", "backward_pass_and_primal": "primal_pass", "compute_pass_and_primal": "primal_pass",
    "decode_primal": "decode", "set_reparametrization": "mode", "set_reparametrization_type": "rtype",
    "set_speculation": "knob", "set_persistent_launches": "knob", "enable_kernel_timing": "knob", "reset_kernel_timing": "knob",
    "prepare_passes": "knob", "invalidate_lower_bounds": "knob", "synchronize": "knob",
    "upload_costs_cold": "cold", "upload_costs_warm": "warm", "set_vectors": "vectors", "zero_pairwise_duals": "zero",
    "set_vectors_diff": "vectors", "set_constants": "consts", "upload_shared_pool": "pool", "upload_duals": "duals", "upload": "reupload", "refused": "refused",
    "lower_bound": "lb", "factor_lower_bounds": "flb", "download_duals": "dl", "labels": "labels",
    "ro_labels": "ro_labels", "ro_vectors": "ro_vectors", "ro_beliefs": "ro_beliefs",
    "window_set_create": "move", "window_set_destroy": "move", "move_windows": "move",
    "path_moves": "relabel", "forest_moves": "relabel", "upload_primal": "relabel",
    "path_set_create": "sets", "forest_set_create": "sets", "path_set_destroy": "sets", "forest_set_destroy": "sets",
}
CLASS_OPS = {c: tuple(o for o, k in OP_CLASS.items() if k == c) for c in STATE + OBSERVING}
NEEDS_MODE = {"compute_pass", "forward_pass", "backward_pass", "forward_pass_and_primal", "backward_pass_and_primal",
              "compute_pass_and_primal", "prepare_passes"}


# ---- models ------------------------------------------------------------------------------------------------------------------
# the keys whose models admit path / forest sets, their moves and upload_primal, with the (H, W) of the colour-major grid that the
# unaries of the lists are taken from (None: lists from the suggested forest cover)
RELABEL_GRIDS = {"rgrid8": (9, 7), "rmixed4": None, "rrows": None, "rlists": (5, 4), "rshift24": (7, 6), "rshift72": (7, 6)}


@functools.lru_cache(maxsize=None)
def base_model(key):
    """the models of the cells, built once per process and never modified"""
    if key == "joined32":          # (compute_primal keeps the peer-minima form: Plan.peer_minima, checked in test_session_host.py)
        return S.grid_model(40, 36, 32, order="colour_major", compute_primal=True)
    if key == "mixed4":
        return MP.m1()
    if key == "rows":
        return RC.rows_graph()
    if key == "deep":
        return RC.mailbox_grid()
    if key == "lists":
        return RC.c5_small()
    if key == "diff40":
        return RP.diff_grid(40)
    if key == "shared32":
        return RP.shared_grid_small(32)
    if key == "rgrid8":            # the lane-group form of the move kernels; dense tables (float tables under the f32 modes)
        return S.grid_model(9, 7, 8, order="colour_major", compute_primal=True)
    if key == "rmixed4":           # SHARED, DIFF and Potts links in one model: the float-table path of the move kernels (tab_flag)
        return MP.m1()
    if key == "rrows":             # the rows layout: a move's rows_refresh is real work
        return RC.rows_graph()
    if key == "rlists":            # a Potts grid (its first factors: move_base) beside labeling-list factors: the rounding code refuses it
        return S.c5_model(5, 4, 4, 12, 6, 3, seed=2, window=12)
    if key in ("rshift24", "rshift72"):      # the models of shift24 / shift72 under keys that admit the relabelling ops
        return base_model(key[1:])
    if key in ("shift24", "shift72"):      # one register per lane and the <= 32 read-out groups | two registers, the > 64 sweep class
        L = int(key[5:])
        return DS.shift_grid(7, 6, L, order="colour_major", compute_primal=True, lengths=(5, L, 2 * L - 1))
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def props(key):
    m = base_model(key)
    mrf = all(t.kind == M.M_UNARY_PAIRWISE for t in m.mtypes)
    vec_types = np.unique(m.f_type[m.f_kind == M.F_VECTOR])
    pw = m.f_kind[m.f_kind != M.F_VECTOR]
    # shift: some factor is DIFF_SHIFT; windows: every pairwise factor is (every unary may be listed in a window set)
    return dict(mrf=mrf, rounds=mrf and bool(np.all(np.asarray(m.ftype_computes_primal)[vec_types] != 0)), pool=m.sh_data is not None,
                diff=m.has_diff, dense=bool(np.any(m.f_kind == M.F_PAIRWISE_DENSE)), rows_layout=key in ("rows", "rrows"), relabel=key in RELABEL_GRIDS,
                shift=bool(np.any(pw == M.F_PAIRWISE_DIFF_SHIFT)), windows=mrf and len(pw) > 0 and bool(np.all(pw == M.F_PAIRWISE_DIFF_SHIFT)))


@functools.lru_cache(maxsize=None)
def _structure_oracle(key):
    return Oracle(RC.oracle_model(base_model(key)))


@functools.lru_cache(maxsize=6)
def model_with_costs(key, seed, strict):
    """the cell's model with the costs of ``seed`` (None: as built); ``strict``: constants that are exactly floats"""
    m = base_model(key)
    if seed is None:
        return MP.float_valued(m) if strict else m
    new = RC.recost_shift(m, seed, float_valued=strict)
    if key == "rgrid8":
        # new costs of this model are multiples of 1/4: sums are exact and minimisers tie, so that "the smallest minimiser" is asked for
        q = lambda x: np.round(np.asarray(x, np.float64) * 4.0) / 4.0
        new = dataclasses.replace(new, const_data=q(new.const_data), dual_data=q(new.dual_data), _keep=[])
    return new


def vectors_of(m):
    return np.flatnonzero((m.f_kind == M.F_VECTOR) & (m.dual_sizes() == m.f_dim0)).astype(np.int32)


def vector_subset(m, seed):
    """about a third of the vector factors in shuffled order, and one row of new values for each"""
    rng = np.random.default_rng(seed)
    v = vectors_of(m)
    f = rng.permutation(v)[:max(1, len(v) // 3)].astype(np.int32)
    return f, rng.random((len(f), int(m.f_dim0[f].max())))


MOVE_FORMS = ("host", "device", "host_costs", "device_costs", "equal", "zero")


def window_list(m, seed):
    """the list of a window set: None (every unary) or the shuffled third of them a read-out lists"""
    return None if seed is None else vector_subset(m, seed)[0]


def window_deltas(dims, seed, form):
    """one delta per listed unary of ``dims[i]`` labels: about half 0, the rest from +-1, +-2, +-(d - 1), +-d, +-(d + 7); from 65 labels
    on both signs of a move with 64 <= |delta| < d are forced into two entries (move_windows_cases.has_hazard).  ``equal``: one of the named
    values, never 0, for every entry; ``zero``: all 0.  No other form gives all 0."""
    dims = np.asarray(dims, np.int64)
    if form == "zero":
        return np.zeros(len(dims), np.int64)
    rng = np.random.default_rng([int(seed), 11])
    named = np.stack([dims * 0 + 1, dims * 0 + 2, dims - 1, dims, dims + 7])
    named = np.concatenate([named, -named])
    if form == "equal":
        return np.full(len(dims), named[int(rng.integers(0, 10)), int(np.argmax(dims))], np.int64)
    out = np.where(rng.random(len(dims)) < 0.5, 0, named[rng.integers(0, 10, len(dims)), np.arange(len(dims))]).astype(np.int64)
    big = np.flatnonzero(dims > 64)
    if len(big) >= 2:
        out[big[-1]] = int(rng.integers(64, dims[big[-1]]))
        out[big[-2]] = -int(rng.integers(64, dims[big[-2]]))
    if not out.any():
        out[0] = 1
    return out


def move_args(m, nominal, lst, seed, form, inf):
    """(listed factors, delta, cost_old, cost_new, stride) of a move_windows step on model ``m``: the costs (forms ..._costs) are
    ``nominal`` (packed like the duals: the unary costs the session gave last) in the old window and move_windows_cases.cost_pair's
    new ones; the device form has a stride above the longest vector"""
    f = np.asarray(RO.unaries(m) if lst is None else lst, np.int32)
    delta = window_deltas(m.f_dim0[f], seed, form)
    if not form.endswith("_costs"):
        return f, delta, None, None, None
    stride = int(m.f_dim0[f].max()) + (5 if form == "device_costs" else 0)
    co, cn = MW.cost_pair(RP.with_duals(m, nominal), f, delta, seed, stride=stride, inf=inf)
    return f, delta, co, cn, stride


def moved_nominal(m, packed, f, delta, cost_new=None):
    """the unary costs a session keeps (``nominal``, the pending ``warm_new``) after a move: gathered by g like the duals; with costs the
    listed rows are cost_new (an entry that is +inf in cost_new was carried: it keeps the gathered value)"""
    out = np.array(packed, np.float64, copy=True)
    doff = m.dual_offsets()
    for i, u in enumerate(f):
        d = int(m.f_dim0[u])
        g = np.clip(np.arange(d) + int(delta[i]), 0, d - 1)
        row = np.asarray(packed[doff[u]:doff[u] + d])[g]
        out[doff[u]:doff[u] + d] = row if cost_new is None else np.where(np.isinf(cost_new[i, :d]), row, cost_new[i, :d])
    return out


@functools.lru_cache(maxsize=16)
def custom_rows(key, seed):
    return random_rows(np.random.default_rng(seed), None, _structure_oracle(key), base_model(key))


def pool_variant(m, variant):
    """pool values by name: "u<seed>" a u01 stream (repool_cases.pool_of); for a pool that is ONE difference vector the truncated
    linear ones of repool_cases (banded / unbanded: the launches of class diff change their kernel)"""
    if variant[1:].isdigit():
        return RP.pool_of(m, int(variant[1:]))
    L = (m.sh_data.shape[0] + 1) // 2
    return RP.tl(L, {"banded": RP.BANDED, "banded2": RP.BANDED_2, "unbanded": RP.UNBANDED}[variant]).reshape(-1).copy()


def original_unaries(m, duals):
    """the packed duals with every pairwise vector zero and every unary theta_u + sum over its messages of m_s (lpmp_decode_primal:
    "with all neighbours theta_u + sum m_s is the original unary"), added in ascending message index"""
    doff = m.dual_offsets()
    out = np.array(duals, np.float64, copy=True)
    for k in range(m.n_messages):
        u, p, s = int(m.m_left[k]), int(m.m_right[k]), int(m.mtypes[int(m.m_type[k])].param)
        d0 = int(m.f_dim0[u])
        a = int(doff[p]) + (0 if s == 0 else int(m.f_dim0[p]))
        out[doff[u]:doff[u] + d0] = out[doff[u]:doff[u] + d0] + duals[a:a + d0]
    out[~RC.vector_mask(m)] = 0.0
    return out


_MEMO = collections.OrderedDict()


def _memo(what, m, duals, extra, fn):
    """a pure numpy statement evaluated once per (costs, duals, arguments): the two sides of a host run ask for the same one"""
    # (a large constant array is told by its identity — the entry keeps it alive —: the costs of a seed are one array for every shadow)
    big = m.const_data.size > 200000
    key = (what, id(m.const_data) if big else zlib.crc32(np.ascontiguousarray(m.const_data).tobytes()),
           0 if m.sh_data is None else zlib.crc32(m.sh_data.tobytes()), m.n_factors, zlib.crc32(np.ascontiguousarray(duals).tobytes()), extra)
    if key not in _MEMO:
        _MEMO[key] = (fn(), m.const_data)          # (the array lives as long as the entry that is keyed by its identity)
        if len(_MEMO) > 8:
            _MEMO.popitem(last=False)
    return _MEMO[key][0]


_LISTS = {}


def _message_lists(m):
    key = (m.n_factors, m.n_messages, zlib.crc32(m.m_left.tobytes()), zlib.crc32(m.m_right.tobytes()), zlib.crc32(m.m_type.tobytes()))
    if key not in _LISTS:
        _LISTS[key] = RO.message_lists(m)
    return _LISTS[key]


def _beliefs(m, duals, factors):
    """readout_cases.beliefs_np(m, duals, factors) with the message lists of the structure made once per model (they read no cost)"""
    lists, doff, coff = _message_lists(m), m.dual_offsets(), m.const_offsets()
    out = np.full((len(factors), max([int(m.f_dim0[f]) for f in factors], default=0)), np.nan)
    for i, u in enumerate(factors):
        out[i, :int(m.f_dim0[u])] = RO.belief_row(m, duals, u, lists[u], doff, coff)
    return out


def unset_labels(m):
    out = np.zeros((m.n_factors, 2), np.int32)
    out[:, 0] = m.f_dim0
    out[:, 1] = np.where(m.f_kind == M.F_VECTOR, 0, m.f_dim1)
    return out


# ---- path and forest moves: the lists of a session and the model a move is stated on ---------------------------------------------
@functools.lru_cache(maxsize=None)
def move_base(key):
    """the unary / pairwise model the moves on ``key`` are stated on: the model itself or, for rlists, the Potts grid that is its
    first factors, factor for factor (tests/test_path_moves_gpu.py test_unlisted_parts_and_a_labeling_list_factor_elsewhere)"""
    m = base_model(key)
    if key != "rlists":
        return m
    H, W = RELABEL_GRIDS[key]
    mg = S.grid_model(H, W, 4, pairwise="potts", order="colour_major", seed=2)
    n = mg.n_factors
    assert np.array_equal(m.f_kind[:n], mg.f_kind) and np.array_equal(m.f_dim0[:n], mg.f_dim0)
    assert np.array_equal(m.const_data[:mg.const_data.shape[0]], mg.const_data) and np.array_equal(m.dual_data[:mg.dual_data.shape[0]], mg.dual_data)
    assert np.array_equal(m.const_offsets()[:n + 1], mg.const_offsets()) and np.array_equal(m.dual_offsets()[:n + 1], mg.dual_offsets())
    return mg


def _signature(m):
    return (m.n_factors, m.n_messages, zlib.crc32(np.ascontiguousarray(m.f_dim0).tobytes()), zlib.crc32(np.ascontiguousarray(m.m_left).tobytes()))


@functools.lru_cache(maxsize=None)
def _relabel_signatures():
    return {_signature(base_model(k)): k for k in RELABEL_GRIDS}


def move_model(key, eff, duals):
    """(model, duals) a move is stated on: ``eff`` (the model the engine computes on) and the duals, or the prefix of both"""
    mg = move_base(key)
    if mg.n_factors == eff.n_factors:
        return eff, duals
    nc, nd = mg.const_data.shape[0], mg.dual_data.shape[0]
    return dataclasses.replace(mg, const_data=np.array(eff.const_data[:nc], np.float64), dual_data=np.array(duals[:nd], np.float64), _keep=[]), np.array(duals[:nd], np.float64)


@functools.lru_cache(maxsize=None)
def structure_plan(key):
    """the host planner on the structure of ``key`` (no cost enters a check of a path or forest list)"""
    return E.Plan(base_model(key))


@functools.lru_cache(maxsize=None)
def suggested_cover(key):
    return E.Plan(move_base(key)).suggest_forests()


def cover_chains(cover):
    """path groups from forest groups: per tree ONE chain, from a deepest member (the lowest index among them) up to the root.  The
    trees of a group are induced and not adjacent, so the chains of a group are legal paths of one group"""
    out = []
    for un, par in cover:
        parent = dict(zip([int(u) for u in un], [int(q) for q in par]))
        best = {}
        for u in sorted(parent):
            walk = [u]
            while parent[walk[-1]] != -1:
                walk.append(parent[walk[-1]])
            if len(walk) > len(best.get(walk[-1], ())):
                best[walk[-1]] = walk
        out.append([best[r] for r in sorted(best)])
    return out


@functools.lru_cache(maxsize=256)
def path_list(key, seed):
    """the groups of a path set, by seed: whole groups (seed % 4 == 0), a seeded subset of the paths (1), partial paths (2), paths of one
    unary (3: the two colours of a grid, the first unary of every chain elsewhere).  Grids: synthetic.grid_paths — rows and columns —;
    other models: cover_chains(suggested_cover)"""
    rng = np.random.default_rng([int(seed), 23])
    hw, form = RELABEL_GRIDS[key], int(seed) % 4
    groups = S.grid_paths(hw[0], hw[1], "colour_major") if hw else cover_chains(suggested_cover(key))
    groups = [[list(p) for p in g] for g in groups]
    if form == 1:
        keep = [[p for p in g if rng.random() < 0.6] for g in groups]
        groups = keep if any(keep) else groups[:1]
    elif form == 2:
        cut = []
        for g in groups:
            cut.append([])
            for p in g:
                a = int(rng.integers(0, len(p)))
                cut[-1].append(p[a:int(rng.integers(a + 1, len(p) + 1))])
        groups = cut
    elif form == 3 and hw:
        var = S.grid_variable_order(hw[0], hw[1], "colour_major")
        groups = [[[int(var[r, c])] for r in range(hw[0]) for c in range(hw[1]) if (r + c) % 2 == k] for k in (0, 1)]
    elif form == 3:
        groups = [[p[:1] for p in g] for g in groups]
    return groups


@functools.lru_cache(maxsize=256)
def forest_list(key, seed):
    """the groups of a forest set: None — the cover of Plan.suggest_forests(); grids: model.forests_from_paths(path_list(key, seed));
    other models: a seeded subset of the cover's groups in shuffled order"""
    if seed is None:
        return suggested_cover(key)
    if RELABEL_GRIDS[key]:
        return M.forests_from_paths(path_list(key, seed))
    cover = suggested_cover(key)
    rng = np.random.default_rng([int(seed), 27])
    order = rng.permutation(len(cover))[:max(1, int(rng.integers(1, len(cover) + 1)))]
    return [cover[int(g)] for g in order]


def primal_for(m, seed, form):
    """the array of an upload_primal step on the unary / pairwise model ``m``: a random label for every unary; ``partly_unset``: about a
    third of the unaries hold their dimension; ``stray``: about a third hold a negative number.  The pairwise slots take the labels of
    the unaries that hold one (path_moves_cases.propagate: whatever is below the dimension)"""
    unaries, links = PM.structure(m)
    r = np.random.default_rng([int(seed), 29])
    pr = unset_labels(m)
    for u in unaries:
        d, x = int(m.f_dim0[u]), r.random()
        pr[u, 0] = int(r.integers(0, d))
        if form == "partly_unset" and x < 1 / 3:
            pr[u, 0] = d
        if form == "stray" and x < 1 / 3:
            pr[u, 0] = -int(r.integers(1, 9))
    return PM.propagate(m, pr, links)


PRIMAL_FORMS = ("random", "partly_unset", "stray")


def refusal_list(key, kind):
    """a list lpmp_path_set_create / lpmp_forest_set_create refuses, from the structure of the model: ``path_set_ring`` — a shortest
    cycle of the unaries as one path; ``path_set_neighbours_in_group`` — two joined unaries as two paths of one group;
    ``forest_set_not_induced`` — the cycle as a chain of parents (its ends are joined: a chord); ``forest_set_no_edge`` — a child
    and a parent that no pairwise factor joins"""
    _, links = PM.structure(move_base(key))
    count = {u: collections.Counter(v for _, _, v in lk) for u, lk in links.items()}
    adj = {u: sorted(v for v, c in count[u].items() if c == 1 and count[v][u] == 1) for u in links}
    if kind == "path_set_neighbours_in_group":
        u = min(u for u in adj if adj[u])
        return [[[u], [adj[u][0]]]]
    if kind == "forest_set_no_edge":
        u = min(adj)
        w = min(v for v in adj if v != u and u not in count[v] and v not in count[u])
        return [(np.array([u, w], np.int32), np.array([-1, u], np.int32))]
    cycle = None
    for root in sorted(adj):                       # a shortest cycle through the lowest unary that lies on one (breadth first)
        prev, queue = {root: None}, [root]
        for u in queue:
            for v in adj[u]:
                if v not in prev:
                    prev[v] = u
                    queue.append(v)
                elif v != prev[u] and cycle is None:
                    a, b = [u], [v]
                    while prev[a[-1]] is not None:
                        a.append(prev[a[-1]])
                    while prev[b[-1]] is not None:
                        b.append(prev[b[-1]])
                    while len(a) > 1 and len(b) > 1 and a[-2] == b[-2]:
                        a.pop(); b.pop()
                    cycle = a[::-1] + b[:-1]
            if cycle:
                break
        if cycle:
            break
    assert cycle and len(cycle) >= 3 and len(set(cycle)) == len(cycle), cycle
    if kind == "path_set_ring":
        return [[cycle]]
    assert kind == "forest_set_not_induced", kind
    return [(np.array(cycle, np.int32), np.array(cycle[1:] + [-1], np.int32))]


# ---- the shadow ----------------------------------------------------------------------------------------------------------------
def refuse(code, what):
    return E.EngineError(code, "shadow: " + what)


class ShadowReadout:
    def __init__(self, sh, factors):
        self.sh, self.gen = sh, sh.gen
        m = sh.raw
        self.factors = [int(f) for f in (RO.unaries(m) if factors is None else factors)]
        self.n = len(self.factors)

    def _enter(self):
        if self.sh.raw is None or self.gen != self.sh.gen:
            raise refuse(ERR_STATE, "the read-out was made for another model")

    def labels(self):
        self._enter()
        return self.sh.labels[self.factors, 0].copy()

    def vectors(self):
        self._enter()
        return RO.vectors_np(self.sh.raw, self.sh.duals(), self.factors)

    def beliefs(self):
        self._enter()
        m = self.sh.raw
        # supported per listed factor: every message of u is LPMP_M_UNARY_PAIRWISE with u as its left factor
        up = np.array([t.kind == M.M_UNARY_PAIRWISE for t in m.mtypes])[m.m_type]
        other = np.zeros(m.n_factors, bool)
        other[m.m_left[~up]] = True
        other[m.m_right] = True
        bad = [u for u in sorted(set(self.factors)) if other[u]]
        if bad:
            raise refuse(ERR_UNSUPPORTED, "beliefs: factor %d " % bad[0])
        m, d = self.sh.eff(), self.sh.duals()
        return _memo("beliefs", m, d, tuple(self.factors), lambda: _beliefs(m, d, self.factors)).copy()

    def close(self):
        pass


class ShadowWindowSet:
    """Engine.window_set stated on the shadow: the list is checked at create, a move is lp_mp_amd.model.move_windows"""

    def __init__(self, sh, factors):
        self.sh, self.gen = sh, sh.gen
        try:
            self.factors, _, _ = M.window_links(sh.raw, factors)
        except M.WindowsUnsupported as ex:
            raise refuse(ERR_UNSUPPORTED, str(ex))
        except ValueError as ex:
            raise refuse(ERR_INVALID, str(ex))
        self.n = len(self.factors)
        self.max_labels = int(sh.raw.f_dim0[self.factors].max()) if self.n else 0

    def move(self, delta=None, cost_old=None, cost_new=None, stride=None):
        if not self.sh._window_set_alive(self):
            raise refuse(ERR_STATE, "the window set was made for another model")
        delta = np.asarray([] if delta is None else delta).reshape(-1)
        if delta.shape[0] != self.n:
            raise ValueError("move: %d deltas expected" % self.n)
        if (cost_old is None) != (cost_new is None):
            raise refuse(ERR_INVALID, "cost_old and cost_new come together")
        if cost_old is not None and (np.shape(cost_old)[1] if stride is None else stride) < self.max_labels:
            raise refuse(ERR_INVALID, "cost_stride is smaller than the longest listed vector")
        if np.any(np.abs(delta.astype(np.int64)) > M.MOVE_DELTA_MAX):
            raise refuse(ERR_INVALID, "a delta beyond +-2^20")
        self.sh._move(self, delta.astype(np.int64), cost_old, cost_new)

    def close(self):
        pass


class ShadowMoveSet:
    """Engine.path_set / Engine.forest_set stated on the shadow: the groups are checked at create by the host planner on the
    structure of the session's model (what it refuses and how is stated by ``_refused`` from the header and by
    tests/test_session_host.py from the planner's text); a move is the numpy reference of its kind"""

    def __init__(self, sh, kind, groups):
        self.sh, self.gen, self.kind, self.groups = sh, sh.gen, kind, groups
        plan = structure_plan(sh.move_key())
        try:
            (plan.path_info if kind == "path" else plan.forest_info)(groups)
        except E.EngineError as ex:
            raise refuse(ex.code, str(ex))
        flat = E.flatten_path_groups(groups) if kind == "path" else E.flatten_forest_groups(groups)
        self.ident = (kind,) + tuple(zlib.crc32(np.ascontiguousarray(x).tobytes()) for x in flat)

    def move(self, rounds=1):
        if not self.sh._move_set_alive(self):
            raise refuse(ERR_STATE, "the %s set was made for another model" % self.kind)
        if rounds < 0:
            raise refuse(ERR_INVALID, "negative number of rounds")
        self.sh._relabel(self, int(rounds))

    def close(self):
        pass


class Shadow:
    """the engine's method names, stated in numpy and on the CPU oracle (the table at the top of this file)"""

    def __init__(self, device=0):
        self.raw, self.o, self.gen = None, None, 0
        self.rtype, self.mode, self.prec = RT_SHARED, None, "f64"
        self.labels, self.schedules = None, []

    # ---- state ----
    def eff(self):
        """the model the engine computes on: under the f32 table modes its dense tables are the widened floats"""
        return self.raw if self.prec == "f64" else self.raw.with_f32_tables()

    def oracle_model(self, m):
        return MP.oracle_model(m) if self.prec != "f64" else RC.oracle_model(m)      # (round, then expand: mixed_precision_cases)

    def duals(self):
        return self.o.duals()

    def _model(self):
        if self.raw is None:
            raise refuse(ERR_STATE, "no model uploaded")

    def _rebuild(self, duals):
        self.o = Oracle(self.oracle_model(RP.with_duals(self.raw, duals)))
        self.o.set_reparametrization_type(self.rtype)
        if self.mode is not None:
            self.o.set_reparametrization(self.mode)

    def _mrf(self):
        return all(t.kind == M.M_UNARY_PAIRWISE for t in self.raw.mtypes)

    # ---- model and costs ----
    def upload(self, model, const_dev=None, dual_dev=None, keep=None, rows_layout=None, table_precision=None):
        prec = "f64" if table_precision is None else table_precision
        if prec != "f64" and rows_layout:
            self.raw, self.o, self.labels, self.schedules, self.mode = None, None, None, [], None
            self.gen += 1
            raise refuse(ERR_UNSUPPORTED, "table precision f32 and the rows layout cannot be combined")
        self.raw, self.prec, self.mode = model, prec, None
        self.gen += 1
        self.schedules = []
        self.labels = unset_labels(model)
        self._rebuild(model.dual_data)

    def upload_costs(self, const=None, duals=None):
        self._model()
        if const is None and duals is None:
            raise refuse(ERR_STATE, "neither constants nor duals given")
        d = self.duals() if duals is None else np.array(duals, np.float64, copy=True)
        if const is not None:
            self.raw = dataclasses.replace(self.raw, const_data=np.ascontiguousarray(const, np.float64), _keep=[])
        self.labels = unset_labels(self.raw)
        self._rebuild(d)

    def set_vectors(self, factors, src, accumulate=False):
        self._model()
        factors = [int(f) for f in factors]
        for f in factors:
            if self.raw.f_kind[f] != M.F_VECTOR:
                raise refuse(ERR_INVALID, "factor %d is not a VECTOR factor" % f)
        if len(set(factors)) != len(factors):
            raise refuse(ERR_INVALID, "listed twice")
        self._rebuild(RC.scatter_rows(self.raw, self.duals(), factors, src, accumulate))

    def zero_pairwise_duals(self):
        self._model()
        self._rebuild(RC.zero_pairwise(self.raw, self.duals()))

    def set_constants(self, factors, src):
        self._model()
        factors = [int(f) for f in factors]
        m = self.raw
        for f in factors:
            if m.f_kind[f] == M.F_VECTOR:
                raise refuse(ERR_INVALID, "factor %d is a VECTOR factor" % f)
        if len(set(factors)) != len(factors):
            raise refuse(ERR_INVALID, "listed twice")
        if self.prec != "f64":
            sizes = m.const_sizes()
            for i, f in enumerate(factors):
                if m.f_kind[f] != M.F_PAIRWISE_DENSE:
                    continue
                row = np.asarray(src[i][:int(sizes[f])], np.float64)
                with np.errstate(over="ignore"):
                    r32 = row.astype(np.float32).astype(np.float64)
                fin = np.isfinite(row)
                bad = (fin & ~np.isfinite(r32)) | ((row != 0) & (np.abs(row) < np.finfo(np.float32).tiny))
                if self.prec == "f32":
                    bad |= r32 != row
                if np.any(bad):
                    raise refuse(ERR_UNSUPPORTED, "table precision: the row of factor %d" % f)
        self.raw = RP.with_rows(m, factors, src)
        self.labels = unset_labels(self.raw)
        self._rebuild(self.duals())

    def upload_shared_pool(self, sh_data=None):
        self._model()
        if sh_data is None or self.raw.sh_data is None:
            raise refuse(ERR_INVALID, "null argument / no pool")
        sh = np.asarray(sh_data, np.float64).reshape(-1)
        if sh.shape != self.raw.sh_data.shape:
            raise ValueError("upload_shared_pool: a pool of %d entries expected" % self.raw.sh_data.shape[0])
        if np.any(np.isnan(sh)):
            raise refuse(ERR_INVALID, "NaN entry")
        self.raw = self.raw.with_pool(sh)
        self.labels = unset_labels(self.raw)
        self._rebuild(self.duals())

    def upload_duals(self, d):
        self._model()
        self._rebuild(d)

    def window_set(self, factors=None):
        self._model()
        return ShadowWindowSet(self, factors)

    def _window_set_alive(self, ws):
        return self.raw is not None and ws.gen == self.gen

    def _move(self, ws, delta, cost_old, cost_new):
        self.raw, d = M.move_windows(self.raw, self.duals(), ws.factors, delta, cost_old, cost_new)
        self.labels = unset_labels(self.raw)
        self._rebuild(d)

    # ---- path and forest moves ----
    def move_key(self):
        """the key among RELABEL_GRIDS whose model has the structure of the uploaded one"""
        return _relabel_signatures()[_signature(self.raw)]

    def path_set(self, groups):
        self._model()
        return ShadowMoveSet(self, "path", groups)

    def forest_set(self, groups):
        self._model()
        return ShadowMoveSet(self, "forest", groups)

    def _move_set_alive(self, ms):
        return self.raw is not None and ms.gen == self.gen

    def _reference(self, m, d, lab, ms, rounds):
        """the labels after the move, from the array ``lab`` of the model ``m`` the move is stated on"""
        ref = PM.path_moves_reference if ms.kind == "path" else FM.forest_moves_reference
        return _memo("moves", m, d, (ms.ident, rounds, zlib.crc32(np.ascontiguousarray(lab).tobytes())), lambda: ref(m, d, lab, ms.groups, rounds)).copy()

    def _relabel(self, ms, rounds):
        m, d = move_model(self.move_key(), self.eff(), self.duals())
        new = self._reference(m, d, self.labels[:m.n_factors].copy(), ms, rounds)
        if self._mrf():
            self.labels = new
        else:               # the array of unset labels: the unaries of the lists get labels, no pairwise slot is written
            un = np.flatnonzero(m.f_kind == M.F_VECTOR)
            self.labels = self.labels.copy()
            self.labels[un, 0] = new[un, 0]

    # ---- passes ----
    def set_reparametrization(self, mode):
        self._model()
        self.mode = int(mode)
        self.o.set_reparametrization(self.mode)

    def set_reparametrization_type(self, rtype):
        self.rtype = int(rtype)
        if self.o is not None:
            self.o.set_reparametrization_type(self.rtype)

    def _mode(self):
        self._model()
        if self.mode is None:
            raise refuse(ERR_STATE, "no reparametrization set")

    def compute_pass(self, n=1):
        self._mode(); self.o.ComputePass(n)

    def forward_pass(self):
        self._mode(); self.o.ComputeForwardPass()

    def backward_pass(self):
        self._mode(); self.o.ComputeBackwardPass()

    def compute_pass_custom(self, *rows):
        self._model(); self.o.compute_pass_custom(*rows)

    def schedule_create(self, factors, om_off, om, mk_off, mk, fuse=False):
        self._model()
        self.schedules.append((factors, om_off, om, mk_off, mk))
        return len(self.schedules) - 1

    def _schedule(self, sid):
        self._model()
        if not (0 <= sid < len(self.schedules)) or self.schedules[sid] is None:
            raise refuse(ERR_INVALID, "unknown schedule id")
        return self.schedules[sid]

    def schedule_run(self, sid):
        self.o.compute_pass_custom(*self._schedule(sid))

    def schedule_destroy(self, sid):
        self._schedule(sid)
        self.schedules[sid] = None

    def _primal(self, call, it):
        self._mode()
        if not self._mrf():
            raise refuse(ERR_UNSUPPORTED, "primal rounding is built for unary / pairwise models")
        call(it)
        self.labels = self.o.primal()

    def forward_pass_and_primal(self, it):
        self._primal(self.o.ComputeForwardPassAndPrimal, it)

    def backward_pass_and_primal(self, it):
        self._primal(self.o.ComputeBackwardPassAndPrimal, it)

    def compute_pass_and_primal(self, it):
        self._primal(self.o.ComputePassAndPrimal, it)

    def decode_primal(self, direction=0, refine=0):
        self._model()
        if direction not in (0, 1) or refine < 0:
            raise refuse(ERR_INVALID, "direction / refine_sweeps")
        if not self._mrf():
            raise refuse(ERR_UNSUPPORTED, "decode: a message that is not a unary-pairwise one")
        m, d = self.eff(), self.duals()
        self.labels = _memo("decode", m, d, (direction, refine), lambda: DC.decode_reference(m, d, self.o.order(direction), refine)).copy()

    # ---- knobs: no value moves ----
    def set_speculation(self, k): pass
    def set_persistent_launches(self, on): pass
    def enable_kernel_timing(self, on): pass
    def reset_kernel_timing(self): pass
    def invalidate_lower_bounds(self): self._model()
    def synchronize(self): pass
    def prepare_passes(self, n): self._mode()

    # ---- observations ----
    def lower_bound(self):
        self._model()
        return self.o.LowerBound()

    def factor_lower_bounds(self):
        self._model()
        m, d = self.eff(), self.duals()
        return _memo("flb", m, d, 0, lambda: np.array([self.o.factor_lower_bound(f) for f in range(m.n_factors)])).copy()

    def download_duals(self):
        self._model()
        return self.duals()

    def _rounding_tables(self):
        """lpmp_download_primal, lpmp_upload_primal, lpmp_check_primal_consistency, lpmp_evaluate_primal need the rounding code's tables"""
        self._model()
        if not self._mrf():
            raise refuse(ERR_UNSUPPORTED, "primal rounding is built for unary / pairwise models")

    def download_primal(self):
        self._rounding_tables()
        return self.labels.copy()

    def upload_primal(self, primal):
        self._rounding_tables()
        self.labels = np.array(primal, np.int32, copy=True)

    def check_primal_consistency(self):
        self._rounding_tables()
        m, lab = self.raw, self.labels
        side = np.array([int(m.mtypes[int(t)].param) for t in m.m_type], np.int64)
        return bool(np.all(lab[m.m_left, 0] == lab[m.m_right, side]))

    def evaluate_primal(self):
        m, lab = self.raw, self.labels
        unset = (lab[:, 0] >= m.f_dim0) | ((m.f_kind != M.F_VECTOR) & (lab[:, 1] >= m.f_dim1))
        if not self.check_primal_consistency() or np.any(unset):
            return np.inf
        e, d = self.eff(), self.duals()
        return _memo("energy", e, d, zlib.crc32(lab.tobytes()), lambda: DC.energy(RP.with_duals(e, original_unaries(m, d)), lab))

    def readout(self, factors=None):
        self._model()
        return ShadowReadout(self, factors)

    def close(self):
        self.o = None


# ---- cells -----------------------------------------------------------------------------------------------------------------------
PRECISIONS = ("f64", "f32", "f32_round")
RELABEL_N = {"relabel": 160, "relabel_lists": 100, "relabel_windows": 188}       # (session lengths: covering_length plus the margin of the other cells)
# models: what the cell's uploads move through; n: session length; seeds: committed seeds; prologue: fixed first steps
CELLS = {
    "joined32": dict(models=("joined32",), n=116, seeds=(0, 1, 2, 3)),
    "mixed4": dict(models=("mixed4",), n=64, seeds=(0, 1, 2, 3, 4, 5)),
    "rows": dict(models=("rows",), n=82, seeds=(0, 1, 2, 3)),
    "deep": dict(models=("deep",), n=90, seeds=(0, 1, 2, 3)),
    "lists": dict(models=("lists",), n=72, seeds=(0, 1, 2, 3)),
    "diffpool": dict(models=("diff40", "shared32"), n=96, seeds=(0, 1, 2, 3), weight={"pool": 3, "consts": 3}),
    "windows": dict(models=("shift24", "shift72"), n=144, seeds=(0, 1, 2, 3), weight={"move": 3, "consts": 3}),
    # path and forest moves, their sets and upload_primal among all other calls.  relabel: the unary / pairwise models (union: a
    # class that only some of its models admit is drawn, too, and a covering block goes to a model that admits all of it);
    # relabel_lists: a model the rounding code refuses; relabel_windows: the window ops and the new ops on 24 and 72 labels
    "relabel": dict(models=("rgrid8", "rmixed4", "rrows"), n=RELABEL_N["relabel"], seeds=(0, 1, 2, 3), union=True, weight={"relabel": 4, "sets": 2}),
    "relabel_lists": dict(models=("rlists",), n=RELABEL_N["relabel_lists"], seeds=(0, 1, 2, 3), weight={"relabel": 4, "sets": 2}),
    "relabel_windows": dict(models=("rshift24", "rshift72"), n=RELABEL_N["relabel_windows"], seeds=(0, 1, 2, 3), weight={"relabel": 4, "sets": 2, "move": 3, "consts": 2}),
}
# (route 3: a window set goes stale on a hop into a model of another kind, and the engine comes back to a DIFF_SHIFT model)
HOP_ROUTES = {0: ("shared32", "joined32", "lists", "diff40"), 1: ("mixed4", "deep", "rows", "shared32"), 2: ("lists", "joined32", "diff40", "rows"),
              3: ("shift24", "deep", "diff40", "shift72"),
              # (route 4: a path set and a forest set go stale on a hop into a model of another kind, and the engine comes back)
              4: ("rshift24", "deep", "rgrid8", "rshift72")}
HOP_SEEDS = tuple(HOP_ROUTES)


def variant(cell, seed):
    """what a session of the cell is run with besides its steps: table precision, borrowed buffers, environment"""
    v = dict(prec="f64", borrowed=False, env={})
    if cell == "joined32":
        v["env"] = {"LPMP_ROT_BANDS": "6"}
        if seed % 2:
            # the smallest limit there is; explicit ticket lists for every pass count (not the periodic template of long calls), so
            # that the chains of a few long calls together exceed it: the prologue of these seeds prepares them
            v["env"].update({"LPMP_CHAIN_CACHE_MB": "1", "LPMP_ROT_EXPLICIT": "1"})
    elif cell == "mixed4":
        v["prec"], v["borrowed"] = PRECISIONS[seed % 3], seed >= 3
    elif cell == "windows":
        v["borrowed"] = seed == 3          # the packed constants a move writes its shifts to are the caller's buffer
    elif cell == "relabel":
        v["prec"] = PRECISIONS[seed % 3]   # (as in mixed4; the rows layout runs on doubles whatever the session asks for)
    elif cell == "relabel_windows":
        v["borrowed"] = seed == 3
    elif cell == "hop":
        v["env"] = {"LPMP_ROT_BANDS": "6"}
        v["prec"] = "f32_round" if seed == 1 else "f64"
    return v


def admissible_ops(key, prec):
    """op names that may be drawn on this model (the refused ones are kinds of the op "refused")"""
    p = props(key)
    ops = {"compute_pass", "forward_pass", "backward_pass", "compute_pass_custom", "schedule_create", "schedule_run", "schedule_destroy",
           "set_reparametrization", "set_speculation", "set_persistent_launches", "enable_kernel_timing", "reset_kernel_timing",
           "prepare_passes", "invalidate_lower_bounds", "synchronize", "upload_costs_cold", "upload_costs_warm", "set_vectors",
           "zero_pairwise_duals", "set_constants", "upload_duals", "upload", "refused", "lower_bound", "factor_lower_bounds",
           "download_duals", "ro_labels", "ro_vectors"}
    if p["mrf"]:
        ops |= {"decode_primal", "set_reparametrization_type", "labels", "ro_beliefs"}
    if p["rounds"]:
        ops |= {"forward_pass_and_primal", "backward_pass_and_primal", "compute_pass_and_primal"}
    if p["pool"]:
        ops.add("upload_shared_pool")
    if p["windows"]:
        ops |= {"window_set_create", "window_set_destroy", "move_windows"}
    if p["relabel"]:
        ops |= {"path_set_create", "path_set_destroy", "forest_set_create", "forest_set_destroy", "path_moves", "forest_moves"}
        ops |= {"upload_primal"} if p["mrf"] else set()
    return ops


def refusal_kinds(key, prec):
    """refusals the header documents, by model: (kind, code)"""
    p = props(key)
    kinds = ["vectors_twice", "vectors_nonvector", "consts_vector", "consts_twice"]
    kinds += ["decode_direction"] if p["mrf"] else ["decode_lists", "beliefs_lists"]
    kinds += ["pool_nan", "pool_size"] if p["pool"] else ["pool_none"]
    if prec != "f64" and p["dense"]:
        kinds.append("consts_f32")
    if p["windows"]:
        kinds += ["move_delta_range", "move_one_cost", "move_stride", "window_set_twice", "window_set_pairwise"]
    if p["relabel"]:
        kinds += ["moves_negative_rounds", "path_set_ring", "path_set_neighbours_in_group", "forest_set_not_induced", "forest_set_no_edge"]
        kinds += [] if p["mrf"] else ["labels_lists", "upload_primal_lists", "primal_pass_lists"]
    return kinds


def admissible_classes(cell):
    keys = CELLS[cell]["models"]
    ops = (set.union if CELLS[cell].get("union") else set.intersection)(*[admissible_ops(k, "f64") for k in keys])
    return [c for c in STATE if any(o in ops for o in CLASS_OPS[c])], [c for c in OBSERVING if any(o in ops for o in CLASS_OPS[c])], ops


# ---- the generator -----------------------------------------------------------------------------------------------------------------
def _euler_pairs(items):
    """a sequence over ``items`` in which every ordered pair of two different ones occurs as neighbours (an Euler circuit of the
    complete digraph, Hierholzer)"""
    out_edges = {a: [b for b in items if b != a] for a in items}
    stack, circuit = [items[0]], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(out_edges[v].pop())
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


@functools.lru_cache(maxsize=None)
def _covering_blocks(cell):
    """per seed of the cell a list of blocks — tuples of (class, op or refusal kind): together they hold every (state-changing,
    observing) pair as neighbours, every ordered pair of cost-changing classes as neighbours, every op three times and every
    refusal kind once.  The ops of a class are taken in turn over the whole cell."""
    st, ob, ops = admissible_classes(cell)
    blocks = [(s, o) for s in st for o in ob]
    cost = [c for c in COST if c in st]
    chain = _euler_pairs(cost)
    blocks += [tuple(chain[i:i + 7]) for i in range(0, len(chain) - 1, 6)]       # pieces overlap by one class: no pair is lost
    blocks += [("mode", "pass")] * len(CELLS[cell]["seeds"])                      # other weights for the very next pass
    kinds = sorted(set().union(*[refusal_kinds(k, "f64") for k in CELLS[cell]["models"]]) | {"destroyed_schedule", "stale_readout"}
                   | ({"stale_window_set"} if "move" in st else set()) | ({"stale_path_set", "stale_forest_set"} if "relabel" in st else set()))
    names = {c: ([o for o in CLASS_OPS[c] if o in ops] if c != "refused" else kinds) for c in st + ob}
    if "move" in st:
        # class move stands for the move itself wherever a pair or the chain names it; the handles get blocks of their own below
        names["move"] = ["move_windows"]
        # "every call after a move is right": each class that changes no cost right behind a move and right before one (the chain
        # above holds the cost-changing ones), with an observation behind the pair
        for s in st:
            if s not in COST and s not in ("reupload", "refused"):
                blocks += [("move", s, "dl"), (s, "move", "lb")]
    for c in st + ob:
        have = sum(b.count(c) for b in blocks)
        blocks += [(c,)] * max(0, (3 if c != "refused" else 1) * len(names[c]) - have)
    turn = collections.Counter()
    named = []
    for b in blocks:
        nb = []
        for c in b:
            nb.append((c, names[c][turn[c] % len(names[c])]))
            turn[c] += 1
        named.append(tuple(nb))
    # messages that are not zero, zeroed while a prepared schedule exists, and the schedule run on them
    named.append((("custom", "schedule_create"), ("pass", "compute_pass"), ("zero", "zero_pairwise_duals"), ("custom", "schedule_run"), ("dl", "download_duals")))
    if cell == "joined32":
        # every state-changing class right behind single passes with a batch of passes that ran ahead open (_Gen.spec_block)
        named += [(("spec", c),) for c in st]
    if "move" in st:
        mv = ("move", "move_windows")
        named += [(("move", "window_set_create"),), (("move", "window_set_destroy"),)] * 3
        # what a move keeps alive or marks stale, used right behind it: a prepared schedule, the labels (unset, decoded anew, rounded
        # anew), the tracked bounds under a directional sweep and next to lpmp_invalidate_lower_bounds
        named += [(("custom", "schedule_create"), ("pass", "compute_pass"), mv, ("custom", "schedule_run"), ("dl", "download_duals")),
                  (("decode", "decode_primal"), mv, ("labels", "labels"), ("decode", "decode_primal"), ("labels", "labels")),
                  (mv, ("primal_pass", "compute_pass_and_primal"), ("labels", "labels"), mv, ("ro_labels", "ro_labels")),
                  (("lb", "lower_bound"), mv, ("dir", "forward_pass"), ("lb", "lower_bound"), mv, ("dir", "backward_pass"), ("flb", "factor_lower_bounds")),
                  (("knob", "invalidate_lower_bounds"), mv, ("lb", "lower_bound"), mv, ("knob", "invalidate_lower_bounds"), ("lb", "lower_bound"))]
    if "relabel" in st:
        named += _relabel_blocks(st, ob, cost)
    rng = np.random.default_rng(zlib.crc32(cell.encode()))
    order = rng.permutation(len(named))
    seeds = CELLS[cell]["seeds"]
    return {s: [named[i] for i in order[k::len(seeds)]] for k, s in enumerate(seeds)}


def _relabel_blocks(st, ob, cost):
    """the fixed blocks of the cells with path and forest moves.  ``mv``: a path move and a forest move in turn, of one round at least;
    ``move_last``: a move on the set that was created or moved last; ``flush``: what a refusal would try first (stale handles, a
    weight mode) comes before the block, so that its steps stand next to each other"""
    turn = [0]

    def mv():
        turn[0] += 1
        return ("relabel", ("path_moves", "forest_moves")[turn[0] % 2])

    flush, last, lab = ("flush", None), ("relabel", "move_last"), ("labels", "labels")
    seen = lab if "labels" in ob else ("ro_labels", "ro_labels")
    out = []
    # every cost-changing class right behind a move, the labels right behind it: they are unset, whatever array they live in
    out += [(flush, mv(), (c, "move_windows" if c == "move" else None), seen) for c in cost]
    if "decode" in st:
        out.append((flush, ("decode", "decode_primal"), mv(), lab))
    if "primal_pass" in st:
        # a rounding sweep after a move does not depend on the moved labels (test_a_rounding_sweep_does_not_depend_on_earlier_labels)
        cpp = ("primal_pass", "compute_pass_and_primal")
        out.append((flush, cpp, mv(), lab, cpp, lab))
    # the duals of the moment: a move, a pass, a move on the same set; tracked bounds are not stale after a move
    out += [(flush, mv(), ("pass", "compute_pass"), last, seen), (flush, mv(), ("pass", "compute_pass"), last, seen)]
    out.append((flush, ("lb", "lower_bound"), mv(), ("dir", "forward_pass"), ("lb", "lower_bound")))
    # an uploaded labelling (every form in turn) is what the next move starts on
    if "labels" in ob:
        out += [(flush, ("relabel", "upload_primal"), mv(), lab)] * len(PRIMAL_FORMS)
    if "move" in st:
        # a set made before a window move moves on the shifts and duals after it: the labels are unset by the window move and clamped
        out += [(flush, ("sets", kind), ("move", "move_windows"), last, lab) for kind in ("path_set_create", "forest_set_create")]
    if "labels" not in ob:
        # a model the rounding code refuses: every refused label call right behind a move leaves the moved labels
        out += [(flush, mv(), ("refused", kind), ("ro_labels", "ro_labels"))
                for kind in ("labels_lists", "labels_lists", "labels_lists", "upload_primal_lists", "primal_pass_lists", "decode_lists")]
    return out


def observe_plan(cell, seed, session):
    """per step: are the duals downloaded and compared after it?  About one state-changing step in four (a knob: one in two), always
    after a refusal, after a move_windows (all delta 0: no byte changes) and after a path or forest move (never a byte changes), never after compute_pass(1) — a download settles a speculative batch, and a batch has to live across the call
    that follows it.  One draw per step index, so a prefix of a session has the prefix of the plan."""
    u = np.random.default_rng([zlib.crc32(cell.encode()), int(seed), 7]).random(len(session))
    out = []
    for (op, a), x in zip(session, u):
        c = OP_CLASS[op]
        out.append(c not in OBSERVING and (c == "refused" or op in ("move_windows", "path_moves", "forest_moves") or (op != "compute_pass" or a[0] != 1) and x < (0.5 if c == "knob" else 0.25)))
    return out


class SpecSim:
    """what lpmp_set_speculation's paragraph says of batches, as a state machine over the steps: when a batch of passes that ran ahead
    is open and whether the caller stands inside it (include/lpmp_engine.h; only the joined32 model with its switches opens one).  The
    generator asks it where a call would meet an open batch; tests/test_session_gpu.py compares its counts with the engine's."""

    def __init__(self):
        self.max_depth = self.n = self.pos = self.run_len = self.learned = self.last_batch = 0
        self.timing, self.persistent, self.rtype, self.mode, self.key = False, True, RT_SHARED, None, None
        self.batches = self.rollbacks = 0

    def usable(self):
        return (self.key == "joined32" and self.max_depth >= 2 and self.rtype == RT_SHARED and self.persistent and not self.timing
                and self.mode in (M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2))

    def inside(self):
        return self.n > 0 and self.pos < self.n

    def _interrupt(self):
        if self.run_len > 0:
            self.learned = self.run_len
        self.run_len = self.last_batch = 0

    def settle(self):
        if self.inside():
            self.rollbacks += 1
        self.n = self.pos = 0
        self._interrupt()

    def _release(self):
        self.n = self.pos = self.run_len = self.learned = self.last_batch = 0

    def step(self, op, a, check=False):
        """(a batch was open, the caller stood inside it) when the step came"""
        before = (self.n > 0, self.inside())
        if op == "upload":
            self._release()
            self.key, self.mode = a[0], None
        elif op == "set_speculation":
            self.settle()
            self.max_depth = min(a[0], 32)
            if self.max_depth < 2:
                self._release()
        elif op == "compute_pass" and a[0] == 1 and self.max_depth >= 2:
            if self.inside():
                self.pos += 1; self.run_len += 1
            else:
                self.n = self.pos = 0
                depth = (self.learned if self.learned > 0 else 2) if self.run_len == 0 else max(2, 2 * self.last_batch)
                depth = min(depth, self.max_depth)
                if self.usable() and depth >= 2:
                    self.n, self.pos, self.last_batch = depth, 1, depth
                    self.batches += 1
                else:
                    self.last_batch = 0
                self.run_len += 1
        elif op in ("lower_bound", "prepare_passes", "reset_kernel_timing"):
            pass
        elif op == "set_reparametrization":
            if a[0] != self.mode:
                self.settle()
            self.mode = a[0]
        elif op == "set_reparametrization_type":
            if a[0] != self.rtype:
                self.settle()
            self.rtype = a[0]
        elif op == "upload_costs_cold":
            self.n = self.pos = 0
            self._interrupt()
        else:
            self.settle()
            if op == "enable_kernel_timing":
                self.timing = bool(a[0])
            if op == "set_persistent_launches":
                self.persistent = bool(a[0])
        if check:
            self.settle()
        return before


def spec_trace(cell, seed, session):
    """SpecSim over a session under its observe plan: per step (open, inside) as the step came, and the machine at the end"""
    sim, out = SpecSim(), []
    for (op, a), chk in zip(session, observe_plan(cell, seed, session)):
        out.append(sim.step(op, a, chk))
    return out, sim


class _Gen:
    """emits steps one by one; keeps the little state that decides what may come next — a pure function of what it emitted"""

    def __init__(self, cell, seed, prec):
        self.cell, self.seed, self.prec0 = cell, seed, prec
        self.rng = np.random.default_rng([zlib.crc32(cell.encode()), seed])
        self.steps = []
        self.key, self.prec, self.mode_set = None, prec, False
        self.live, self.dead, self.n_slots = [], [], 0
        self.turn = {}
        self.uploads = 0
        self.stale = False           # handles of the previous model not yet tried
        self.tried_f32 = False
        self.sim = SpecSim()         # follows every step pushed (with the observe plan of the session)
        self.u = np.random.default_rng([zlib.crc32(cell.encode()), int(seed), 7]).random(4096)
        self.mode, self.rtype = None, RT_SHARED
        self.warm_diff = False       # the difference new - old of the last warm start is still to come
        self.warms = 0
        self.wlive, self.w_slots, self.w_old = {}, 0, 0      # live window sets {slot: lists every unary}; sets of the previous model not yet tried
        self.plive, self.p_slots, self.p_old = {}, 0, []     # live path / forest sets {slot: kind}; kinds of those of the previous model not yet tried
        self.last_set = None                                 # (kind, slot) of the set created or moved last

    def set_create(self, kind, list_seed):
        self.push(kind + "_set_create", self.p_slots, list_seed)
        self.plive[self.p_slots] = kind
        self.last_set = (kind, self.p_slots)
        self.p_slots += 1
        return self.p_slots - 1

    def set_of(self, kind):
        """a live set of the kind (one is made when there is none)"""
        slots = sorted(s for s, k in self.plive.items() if k == kind)
        if not slots:
            return self.set_create(kind, self._seed())
        return int(slots[int(self.rng.integers(0, len(slots)))])

    def flush(self):
        """what a refusal would try first comes now: the stale handles of the model before, a weight mode for the sweeps"""
        if self.stale or self.w_old or self.p_old:
            self.emit_class("refused", "vectors_twice")
        self.need_mode()

    def window_set_create(self, every):
        self.push("window_set_create", self.w_slots, None if every else self._seed())
        self.wlive[self.w_slots] = every
        self.w_slots += 1
        return self.w_slots - 1

    def move_windows(self, form):
        slots = sorted(s for s, every in self.wlive.items() if every or form != "equal")
        if not slots:
            slots = [self.window_set_create(True)]
        inf = form.endswith("_costs") and bool(self._next("inf", (True, False, False)))
        self.push("move_windows", int(slots[int(self.rng.integers(0, len(slots)))]), self._seed(), form, inf)

    def _next(self, what, options):
        i = self.turn.get(what, int(self.rng.integers(0, 1 << 16)))
        self.turn[what] = i + 1
        return options[i % len(options)]

    def _seed(self):
        return int(self.rng.integers(1, 1 << 30))

    def push(self, op, *args):
        self.steps.append((op, tuple(args)))
        i = len(self.steps) - 1
        self.sim.step(op, tuple(args), self._check(i))
        if op == "set_reparametrization":
            self.mode, self.mode_set = args[0], True
        if op == "set_reparametrization_type":
            self.rtype = args[0]

    def _check(self, i):
        op, a = self.steps[i]
        c = OP_CLASS[op]
        return c not in OBSERVING and (c == "refused" or op in ("move_windows", "path_moves", "forest_moves") or (op != "compute_pass" or a[0] != 1) and self.u[i] < (0.5 if c == "knob" else 0.25))

    def spec_block(self, c, want=None):
        """speculation usable, single passes until the caller stands inside a batch, then a call of class ``c`` and a download"""
        if self.sim.max_depth < 2:
            self.push("set_speculation", 8)
        if self.sim.timing:
            self.push("enable_kernel_timing", False)
        if not self.sim.persistent:
            self.push("set_persistent_launches", True)
        if self.rtype != RT_SHARED:
            self.push("set_reparametrization_type", RT_SHARED)
        if not self.mode_set or self.mode not in (M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2):
            self.push("set_reparametrization", ANISO)
        for _ in range(6):
            self.push("compute_pass", 1)
            if self.sim.inside():
                break
        if c == "pass":
            self.push("compute_pass", int(self._next("n_spec", (3, 2, 5))))
        elif c == "mode":
            self.push("set_reparametrization", int(self._next("mode_spec", (M.REPAM_UNIFORM, M.REPAM_DAMPED_UNIFORM))))
        elif c == "rtype":
            self.push("set_reparametrization_type", RT_RESIDUAL)
        elif c == "custom":
            self.emit_class(c, self._next("custom_spec", ("compute_pass_custom", "schedule_create")))
        elif c == "refused":
            self.emit_class(c, self._next("refused_spec", ("vectors_twice", "consts_vector", "decode_direction", "pool_none", "pool_nan")))
        else:
            self.emit_class(c, want)
        self.push("download_duals")

    def restore_speculation(self):
        """the random tail keeps passes that run ahead possible most of the time: a switch that rules them out is set back"""
        if self.key != "joined32":
            return
        if self.sim.max_depth < 2:
            self.push("set_speculation", int(self._next("spec_on", (8, 2, 4))))
        if self.sim.timing:
            self.push("enable_kernel_timing", False)
        if not self.sim.persistent:
            self.push("set_persistent_launches", True)
        if self.rtype != RT_SHARED:
            self.push("set_reparametrization_type", RT_SHARED)

    def upload(self, key, recost=True, prec=None):
        p = props(key)
        prec = self.prec0 if prec is None else prec
        if p["rows_layout"]:
            prec = "f64"
        # every third upload of a model with dense tables first asks for float tables under the rows layout: refused, no model left
        refused_first = p["dense"] and self.uploads % 3 == 1
        if not p["mrf"] and self.rtype != RT_SHARED:      # the send rule stays across an upload: only SHARED is drawn on such a model
            self.push("set_reparametrization_type", RT_SHARED)
        self.push("upload", key, self._seed() if recost and self.uploads else None, prec, self._seed(), refused_first)
        self.stale = self.uploads > 0
        self.uploads += 1
        self.key, self.prec, self.mode_set = key, prec, False
        self.live, self.dead = [], []
        self.warm_diff = False
        self.w_old, self.wlive = len(self.wlive), {}
        self.p_old, self.plive, self.last_set = [self.plive[s] for s in sorted(self.plive)], {}, None

    def need_mode(self):
        if not self.mode_set:
            self.push("set_reparametrization", int(self._next("mode", MODES)))

    def emit_class(self, c, want=None):
        """one step of class ``c`` (``want``: this op / refusal kind where it can be drawn now), after whatever it needs first"""
        if c == "flush":
            return self.flush()
        ops = [o for o in CLASS_OPS[c] if o in admissible_ops(self.key, self.prec)]
        if c == "sets":
            op = want if want in ops else self._next(c, ("path_set_create", "forest_set_create", "path_set_destroy", "forest_set_create", "forest_set_destroy", "path_set_create"))
            kind = op.split("_")[0]
            if op.endswith("_create"):
                # (a forest set: the suggested cover every other time)
                self.set_create(kind, None if kind == "forest" and self._next("cover", (True, False)) else self._seed())
            else:
                if len([s for s, k in self.plive.items() if k == kind]) < 2:      # (one set of a kind stays: a move never waits for one)
                    self.set_create(kind, self._seed())
                slots = sorted(s for s, k in self.plive.items() if k == kind)
                slot = slots[int(self.rng.integers(0, len(slots)))]
                del self.plive[slot]
                self.last_set = None if self.last_set == (kind, slot) else self.last_set
                self.push(op, int(slot))
            return
        if c == "relabel":
            if want == "move_last" and self.last_set is not None:
                kind, slot = self.last_set
                self.push(kind + "_moves", int(slot), int(self._next("rounds_w", (1, 2, 1, 3))))
                return
            op = want if want in ops else self._next(c, [o for o in ("path_moves", "forest_moves", "upload_primal", "forest_moves", "path_moves") if o in ops])
            if op == "upload_primal":
                self.push(op, self._seed(), self._next("primal_form", PRIMAL_FORMS))
                return
            kind = op.split("_")[0]
            slot = self.set_of(kind)
            # (a move a block asks for does at least one round)
            self.push(op, slot, int(self._next("rounds_w", (1, 2, 1, 3)) if want else self._next("rounds", (1, 2, 0, 1, 3, 1))))
            self.last_set = (kind, slot)
            return
        if c == "custom":
            op = want if want in ops else self._next(c, ops)
            if op in ("schedule_run", "schedule_destroy") and not self.live:
                self.push("schedule_create", self.n_slots, self._seed(), bool(self.rng.integers(0, 2)))
                self.live.append(self.n_slots); self.n_slots += 1
            if op == "compute_pass_custom":
                self.push(op, self._seed())
            elif op == "schedule_create":
                self.push(op, self.n_slots, self._seed(), bool(self.rng.integers(0, 2)))
                self.live.append(self.n_slots); self.n_slots += 1
            elif op == "schedule_run":
                self.push(op, int(self.live[int(self.rng.integers(0, len(self.live)))]))
            else:
                slot = self.live.pop(int(self.rng.integers(0, len(self.live))))
                self.dead.append(slot)
                self.push(op, int(slot))
            return
        if c == "reupload":
            keys = CELLS[self.cell]["models"] if self.cell in CELLS else (self.key,)
            precs = (self.prec0, "f64") if self.prec0 != "f64" else ("f64",)
            # (the windows cell goes to its other model every time: both are reached with two uploads)
            key = [k for k in keys if k != self.key][0] if self.cell in ("windows", "relabel_windows") else self._next("key", keys)
            self.upload(key, prec=self._next("prec", precs))
            return
        if c == "move":
            op = want if want in ops else self._next(c, ("move_windows", "move_windows", "window_set_create", "move_windows", "move_windows",
                                                         "window_set_destroy", "move_windows"))
            if op == "window_set_create":
                self.window_set_create(bool(self._next("w_every", (False, True, False))))
            elif op == "window_set_destroy":
                if len(self.wlive) < 2:                                # (one set stays: a move never waits for one)
                    self.window_set_create(False)
                slot = sorted(self.wlive)[int(self.rng.integers(0, len(self.wlive)))]
                del self.wlive[slot]
                self.push(op, int(slot))
            else:
                self.move_windows(self._next("form", ("host", "device_costs", "equal", "device", "host_costs", "host", "zero", "device", "host_costs", "device_costs")))
            return
        if c == "refused":
            kinds = refusal_kinds(self.key, self.prec) + ["destroyed_schedule"] + (["stale_readout"] if self.uploads >= 2 else [])
            kinds += ["stale_window_set"] if self.w_old else []
            kinds += sorted({"stale_%s_set" % k for k in self.p_old})
            kind = want if want in kinds else self._next(c, kinds)
            if kind in ("stale_path_set", "stale_forest_set"):
                self.p_old.remove(kind.split("_")[1])                         # (the one the step itself tries)
            for k in self.p_old:                                               # the sets of the previous model are tried once after every upload
                self.push("refused", "stale_%s_set" % k, 0)
            self.p_old = []
            if self.w_old and kind != "stale_window_set":          # a set of the previous model is tried once after every upload
                self.push("refused", "stale_window_set", 0)
                self.w_old -= 1
            if kind == "stale_window_set":
                self.w_old -= 1
            if kind.startswith("move_"):
                self.push("refused", kind, int(sorted(self.wlive)[int(self.rng.integers(0, len(self.wlive)))]))
                return
            if kind in ("stale_path_set", "stale_forest_set"):
                self.push("refused", kind, 0)
                return
            if kind == "moves_negative_rounds":
                k = self._next("neg_kind", ("path", "forest"))
                self.push("refused", kind, self.set_of(k))
                return
            if kind == "primal_pass_lists":
                self.need_mode()
            if kind == "labels_lists":                                 # download_primal, evaluate_primal, check_primal_consistency in turn
                self.push("refused", kind, int(self._next("labels_lists", (0, 1, 2))))
                return
            if self.stale and kind != "stale_readout":              # handles of the previous model are tried once after every move
                self.push("refused", "stale_readout", self._seed())
            extra = "consts_f32" in kinds and not self.tried_f32 and kind not in ("consts_f32", "stale_readout")      # once per session with float tables
            self.stale = False
            self.tried_f32 |= kind == "consts_f32"
            if kind == "destroyed_schedule" and not self.dead:
                self.push("schedule_create", self.n_slots, self._seed(), False)
                self.push("schedule_destroy", self.n_slots)
                self.dead.append(self.n_slots); self.n_slots += 1
            self.push("refused", kind, int(self.dead[-1]) if kind == "destroyed_schedule" else self._seed())
            if extra:
                self.push("refused", "consts_f32", self._seed())
                self.tried_f32 = True
            return
        op = want if want in ops else self._next(c, ops)
        if op in NEEDS_MODE:
            self.need_mode()
        if op == "compute_pass":
            self.push(op, int(self._next("n", (1, 2, 3, 5, 1, 1))))
        elif c == "primal_pass":
            self.push(op, len(self.steps) + 1)                      # the iteration: time stamps never repeat and never decrease
        elif op == "decode_primal":
            self.push(op, int(self.rng.integers(0, 2)), int(self._next("refine", (0, 1, 2))))
        elif op == "set_reparametrization":
            self.push(op, int(self._next("mode", MODES)))
        elif op == "set_reparametrization_type":
            self.push(op, int(self._next("rtype", (RT_RESIDUAL, RT_SHARED))))
        elif op == "set_speculation":
            self.push(op, int(self._next("spec", (8, 2, 0, 8))))
        elif op in ("set_persistent_launches", "enable_kernel_timing"):
            self.push(op, bool(self._next(op, (False, True, True))))
        elif op == "prepare_passes":
            self.push(op, int(self._next("prep", (2, 3, 5))))
        elif op in ("upload_costs_cold", "upload_costs_warm", "set_constants"):
            self.push(op, self._seed())
            if op == "upload_costs_warm":
                self.warms += 1
                self.warm_diff = self.warms % 2 == 1
            elif op == "upload_costs_cold":
                self.warm_diff = False
        elif op == "set_vectors":
            self.push(op, self._seed(), bool(self._next("acc", (False, True))))
        elif op == "upload_shared_pool":
            one_vector = self.key == "diff40"
            self.push(op, self._next("pool", ("unbanded", "banded", "u7", "banded2", "unbanded", "u9") if one_vector else ("u%d" % self._seed(),)))
        else:
            self.push(op)

    def random_class(self):
        union = self.cell in CELLS and CELLS[self.cell].get("union")      # (what the model of the moment admits, and a re-upload)
        st, ob, _ = admissible_classes(self.cell) if self.cell in CELLS and not union else (None, None, None)
        if st is None:
            ops = admissible_ops(self.key, self.prec)
            st = [c for c in STATE if (union or c != "reupload") and any(o in ops for o in CLASS_OPS[c])]
            ob = [c for c in OBSERVING if any(o in ops for o in CLASS_OPS[c])]
        w = CELLS.get(self.cell, {}).get("weight", {})
        cls = st + ob + ["pass"] * 3
        p = np.array([w.get(c, 1) for c in cls], np.float64)
        return cls[int(self.rng.choice(len(cls), p=p / p.sum()))]


def _block_key(g, block):
    """a cell whose models admit different classes (union): the key of a model that admits every step of the block — the model of the
    moment where it does"""
    def admits(key):
        ops, kinds = admissible_ops(key, "f64"), refusal_kinds(key, "f64")
        for c, want in block:
            if c in ("flush", "spec"):
                continue
            if c == "refused":
                if want in set().union(*[refusal_kinds(k, "f64") for k in CELLS[g.cell]["models"]]) and want not in kinds:
                    return False
            elif not any(o in ops for o in CLASS_OPS[c]) or (want in OP_CLASS and want not in ops):
                return False
        return True
    keys = [k for k in CELLS[g.cell]["models"] if admits(k)]
    return g.key if g.key in keys else g._next("block_key", keys)


def _after_block(g, state):
    if g.key is not None and props(g.key)["relabel"] and not g.plive:
        # a path set and a forest set behind the block of an upload — a move never waits for one —: made before the first window move
        g.set_create("path", g._seed())
        g.set_create("forest", None)
    if g.key is not None and props(g.key)["windows"] and not g.wlive:
        # a set of every unary behind the block of an upload — a move never waits for one —, and one move of the new model's windows
        # between two passes before anything else happens to it
        g.window_set_create(True)
        g.need_mode()
        g.push("compute_pass", 1); g.move_windows(g._next("first_form", ("host", "device_costs", "device", "host_costs"))); g.push("compute_pass", 1)
    if g.warm_diff:                                 # every other warm start is followed, a step or two later, by its new - old
        g.push("set_vectors_diff")
        g.warm_diff = False
    if g.key == "joined32":
        s = g.sim
        off = s.max_depth < 2 or s.timing or not s.persistent or g.rtype != RT_SHARED
        state["off"] = state.get("off", 0) + 1 if off else 0
        if state["off"] >= 2:
            g.restore_speculation()
            state["off"] = 0


def _cell_steps(cell, seed, n):
    g = _Gen(cell, seed, variant(cell, seed)["prec"])
    # (the windows cell starts on its 24-label model with even seeds and on its 72-label model with odd ones)
    g.upload(CELLS[cell]["models"][seed % 2 if cell in ("windows", "relabel_windows") else seed % 3 if cell == "relabel" else 0], recost=False)
    if cell in ("joined32", "deep"):
        g.push("set_reparametrization", ANISO)
    g.need_mode()
    if cell == "joined32":
        # passes that run ahead, and a call that stops inside the second batch (2, then 4): batches > 0, rollbacks > 0, peer minima
        for op, a in (("set_speculation", (8,)), ("compute_pass", (1,)), ("compute_pass", (1,)), ("compute_pass", (1,)), ("lower_bound", ()),
                      ("forward_pass", ()), ("compute_pass", (3,)), ("compute_pass", (2,)), ("compute_pass", (5,)), ("download_duals", ())):
            g.push(op, *a)
        if "LPMP_CHAIN_CACHE_MB" in variant(cell, seed)["env"]:
            # chains of long calls until the least recently used ones have to go, then calls whose chains went
            for k in (31, 30, 29, 28, 27, 26):
                g.push("prepare_passes", k)
            g.push("compute_pass", 3); g.push("compute_pass", 2); g.push("lower_bound")
    if cell == "deep":
        g.push("forward_pass"); g.push("compute_pass", 1); g.push("download_duals")
    if cell == "diffpool":
        # the vector of the upload is banded: a pass on it, a pass after the swap to an unbanded one
        g.push("compute_pass", 1); g.push("upload_shared_pool", "unbanded"); g.push("forward_pass"); g.push("lower_bound")
    if cell == "windows":
        # timed launches of the shifted kernel (the count Reach reads), and a move between two passes before anything else happened
        g.push("enable_kernel_timing", True)
        _after_block(g, {})
        g.push("lower_bound")
    if cell.startswith("relabel"):
        # the sets of the upload, and one move of each kind on labels that are unset before anything else happened
        _after_block(g, {})
        g.emit_class("relabel", "path_moves"); g.emit_class("ro_labels"); g.emit_class("relabel", "forest_moves"); g.emit_class("ro_labels")
    blocks = list(_covering_blocks(cell)[seed])
    state = {}
    while blocks if n is None else len(g.steps) < n:
        block = blocks.pop(0) if blocks else ((g.random_class(), None),)
        if block[0][0] == "spec":
            if g.key == "joined32":
                g.spec_block(block[0][1])
        else:
            key = _block_key(g, block) if CELLS[cell].get("union") else g.key
            if key != g.key:
                g.upload(key)
                _after_block(g, state)
            for c, want in block:
                g.emit_class(c, want)
        _after_block(g, state)
    return g.steps


def _hop_steps(seed, n):
    g = _Gen("hop", seed, variant("hop", seed)["prec"])
    state = {}
    for k, key in enumerate(HOP_ROUTES[seed]):
        had_slot = bool(g.live or g.dead)
        g.upload(key, recost=k > 0)
        if k > 0:
            g.emit_class("refused", "stale_readout")                  # the read-outs of the previous model
            if had_slot:
                g.push("refused", "stale_schedule", 0)
        g.need_mode()
        if props(key)["windows"] or props(key)["relabel"]:          # the set of the upload moves once at least before the next hop
            _after_block(g, state)
        if props(key)["relabel"]:
            g.emit_class("relabel", "path_moves"); g.emit_class("relabel", "forest_moves"); g.emit_class("ro_labels")
        g.push("schedule_create", g.n_slots, g._seed(), False)       # a handle for the next move to try
        g.live.append(g.n_slots); g.n_slots += 1
        spec = [g._next("hop_spec", ("cold", "vectors", "consts", "decode", "custom", "warm", "zero", "duals", "knob", "refused"))
                for _ in range(3)] if key == "joined32" else []
        for j in range(int(g.rng.integers(15, 21)) - 4 * len(spec)):
            g.emit_class(g.random_class())
            _after_block(g, state)
            if spec and j % 2 == 1:
                g.spec_block(spec.pop())
        g.emit_class("dl")
    return g.steps


def steps(cell, seed, n=None):
    """the session (cell, seed) as a list of (op, args): a pure function of its arguments; the first k steps of a longer session
    are the session of length k"""
    if cell == "hop":
        full = _hop_steps(seed, n)
        return full if n is None else full[:n]
    n = CELLS[cell]["n"] if n is None else n
    return _cell_steps(cell, seed, n)[:n]


def covering_length(cell, seed):
    """steps until the covering list of the session has been emitted (its length must not be cut below this)"""
    return len(_cell_steps(cell, seed, None))


def sessions():
    """(cell, seed) of every committed session but the hops"""
    return [(c, s) for c in CELLS for s in CELLS[c]["seeds"]]


# ---- the runner ------------------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    index = None          # the step the error names


class _Side:
    """one engine (or a shadow in an engine's place) with the handles of the session: schedule ids by slot, read-outs by upload"""

    def __init__(self, target, borrowed=False):
        self.t, self.borrowed = target, borrowed
        self.ids, self.readouts, self.old_readouts = {}, None, None
        self.stale_id = None
        self.keep = None
        self.wsets, self.old_wsets = {}, []          # window sets by slot; those of the model before, not yet tried
        self.psets, self.old_psets = {}, []          # (kind, path or forest set) by slot; those of the model before, not yet tried

    def close(self):
        for _, w in list(self.psets.values()) + self.old_psets:
            w.close()
        self.psets, self.old_psets = {}, []
        for r in (self.readouts or ()) + (self.old_readouts or ()):
            r.close()
        self.readouts = self.old_readouts = None
        for w in list(self.wsets.values()) + self.old_wsets:
            w.close()
        self.wsets, self.old_wsets = {}, []


class Reach:
    """what a session on a real engine reached of the state its cell is about (asserted by tests/test_session_gpu.py)"""

    def __init__(self):
        self.peer_minima = self.chain_launches = self.batches = self.rollbacks = 0
        self.cache_max = 0
        self.evictions = 0
        self.banded = self.full = self.rows = False
        self.deep_chain_passes = 0           # passes of a deep schedule planned as ONE persistent launch, run with timing off
        self._timing = False
        self.precisions = set()
        self._cache = 0
        self.moves = self.window_sets = 0     # move_windows / window_set_create steps done (run() checks schedules_built around each)
        self.shift_launches = 0               # timed launches of sweep_diff_shift_kernel
        self.models = set()                   # keys uploaded
        self.lb_rel_max = 0.0                 # largest |lower_bound - oracle's| / max(1, |oracle's|) seen (the limit is LB_RTOL)
        # path_moves / forest_moves steps done, path and forest sets created (run() checks schedules_built around each), moves done while
        # every label was unset, moves on a set that was made before the last move_windows of its model
        self.path_moves = self.forest_moves = self.move_sets = self.moves_on_unset = self.moves_behind_windows = 0

    def before_reset(self, e):
        st = e.speculation_stats()
        self.batches, self.rollbacks = max(self.batches, st["batches"]), max(self.rollbacks, st["rollbacks"])
        self.peer_minima += e.peer_minima_launches()
        timing = e.kernel_timing()
        self.chain_launches += sum(v.get("chain_launches", 0) for v in timing.values())
        self.shift_launches += sum(v.get("shift_launches", 0) for v in timing.values())

    def after_step(self, e, op, args, mode):
        if op == "enable_kernel_timing":
            self._timing = bool(args[0])
        if OP_CLASS[op] in ("pass", "dir") and mode is not None and not self._timing and e.persistent_launches:
            # (with timing on a deep schedule runs launch by launch, and the chain executor keeps no counter of its own: the plan says
            # how the sweep is run, as tests/test_recost_gpu.py test_deep_schedule_as_a_chain_with_the_mailbox asserts it)
            ci = e.plan.chain_info(M.FORWARD, mode)
            self.deep_chain_passes += int(ci["n_chains"] == 1 and ci["mailbox_rows"] > 0)
        st = e.speculation_stats()
        self.batches, self.rollbacks = max(self.batches, st["batches"]), max(self.rollbacks, st["rollbacks"])
        b = e.chain_cache_bytes()
        if b < self._cache and op != "upload":
            self.evictions += 1
        self._cache = b
        self.cache_max = max(self.cache_max, b)
        if op == "upload":
            self.models.add(args[0])
            self.rows |= bool(e.rows_layout)
            self.precisions.add(e.table_precision())
        if OP_CLASS[op] in ("pass", "dir") and mode is not None and e.model.has_diff:
            for d in (0, 1):
                info = e.plan.diff_band_info(d, mode)
                self.banded |= info["band_launches"] > 0
                self.full |= info["diff_launches"] > info["band_launches"]


def _upload(side, m, prec, rows_layout):
    t = side.t
    if side.borrowed and isinstance(t, E.Engine):
        import torch
        c = torch.from_numpy(np.ascontiguousarray(m.const_data)).cuda()
        d = torch.from_numpy(np.ascontiguousarray(m.dual_data)).cuda()
        torch.cuda.synchronize()
        t.upload(m, const_dev=c.data_ptr(), dual_dev=d.data_ptr(), keep=(c, d), rows_layout=rows_layout, table_precision=prec)
        side.keep = (c, d)
    else:
        t.upload(m, rows_layout=rows_layout, table_precision=prec)
        side.keep = None


def _expect(code, call):
    """the call is refused with that code (a ValueError of the Python binding: code "ValueError")"""
    try:
        call()
    except E.EngineError as ex:
        return ex.code == code, "EngineError %s: %s" % (ex.code, ex)
    except ValueError as ex:
        return code == "ValueError", "ValueError: %s" % ex
    return False, "no error"


def _refused(side, sh, kind, arg):
    """(code, call) of a refusal the header documents; ``sh``: the shadow, read for the structure of the current model only"""
    t, m = side.t, sh.raw
    vec, pw = vectors_of(m), np.flatnonzero(m.f_kind != M.F_VECTOR).astype(np.int32)
    L = int(m.f_dim0[vec].max())
    if kind == "vectors_twice":
        return ERR_INVALID, lambda: t.set_vectors([vec[0], vec[-1], vec[0]], np.ones((3, L)))
    if kind == "vectors_nonvector":
        return ERR_INVALID, lambda: t.set_vectors([vec[0], pw[0]], np.ones((2, L)))
    if kind in ("consts_vector", "consts_twice"):
        f = [pw[0], vec[0]] if kind == "consts_vector" else [pw[0], pw[-1], pw[0]]
        return ERR_INVALID, lambda: t.set_constants(f, np.ones((3, int(m.const_sizes().max()))))
    if kind == "consts_f32":
        dense = np.flatnonzero(m.f_kind == M.F_PAIRWISE_DENSE).astype(np.int32)
        f = [dense[arg % len(dense)], pw[0]] if pw[0] != dense[arg % len(dense)] else [dense[arg % len(dense)]]
        rows = RP.rows_for(m, f, arg, float_valued=True)
        rows[0, 3] = 0.1 if sh.prec == "f32" else 1e300              # not a float / beyond float's range
        return ERR_UNSUPPORTED, lambda: t.set_constants(f, rows)
    if kind == "decode_direction":
        return ERR_INVALID, lambda: t.decode_primal(2, 0)
    if kind == "decode_lists":
        return ERR_UNSUPPORTED, lambda: t.decode_primal(arg % 2, 0)
    if kind == "beliefs_lists":
        return ERR_UNSUPPORTED, lambda: side.readouts[1].beliefs()
    if kind == "pool_none":
        return ERR_INVALID, lambda: t.upload_shared_pool(np.ones(4))
    if kind == "pool_nan":
        sh_new = RP.pool_of(m, arg)
        sh_new[(arg % len(sh_new)) // 2 + len(sh_new) // 2 - 1] = np.nan          # in the second half: a half-written pool would show
        return ERR_INVALID, lambda: t.upload_shared_pool(sh_new)
    if kind == "pool_size":
        return "ValueError", lambda: t.upload_shared_pool(np.ones(m.sh_data.shape[0] + 1))
    if kind == "destroyed_schedule":
        return ERR_INVALID, lambda: t.schedule_run(side.ids[arg])
    if kind == "stale_schedule":
        return ERR_INVALID, lambda: t.schedule_run(side.stale_id)
    if kind == "stale_readout":
        return ERR_STATE, lambda: side.old_readouts[arg % 2].vectors()
    if kind == "stale_window_set":
        ws = side.old_wsets[0]
        return ERR_STATE, lambda: ws.move(np.ones(ws.n, np.int32))
    if kind in ("stale_path_set", "stale_forest_set"):
        ms = [w for k, w in side.old_psets if k == kind.split("_")[1]][0]
        return ERR_STATE, lambda: ms.move(1)
    if kind == "moves_negative_rounds":
        return ERR_INVALID, lambda: side.psets[arg][1].move(-1)
    # lpmp_path_set_create / lpmp_forest_set_create, the last group of their refusals: "LPMP_ERR_INVALID, naming the entries"
    if kind in ("path_set_ring", "path_set_neighbours_in_group"):
        return ERR_INVALID, lambda: t.path_set(refusal_list(sh.key, kind))
    if kind in ("forest_set_not_induced", "forest_set_no_edge"):
        return ERR_INVALID, lambda: t.forest_set(refusal_list(sh.key, kind))
    if kind == "labels_lists":
        return ERR_UNSUPPORTED, (t.download_primal, t.evaluate_primal, t.check_primal_consistency)[arg % 3]
    if kind == "upload_primal_lists":
        return ERR_UNSUPPORTED, lambda: t.upload_primal(unset_labels(m))
    if kind == "primal_pass_lists":
        return ERR_UNSUPPORTED, lambda: (t.forward_pass_and_primal, t.backward_pass_and_primal, t.compute_pass_and_primal)[arg % 3](arg)
    if kind == "window_set_twice":
        return ERR_INVALID, lambda: t.window_set([vec[0], vec[-1], vec[0]])
    if kind == "window_set_pairwise":
        return ERR_INVALID, lambda: t.window_set([vec[0], pw[0]])
    if kind.startswith("move_"):
        ws = side.wsets[arg]
        one, co = np.ones(ws.n, np.int32), np.ones((ws.n, ws.max_labels))
        if kind == "move_delta_range":
            one[-1] = M.MOVE_DELTA_MAX + 1
            return ERR_INVALID, lambda: ws.move(one)
        if kind == "move_one_cost":
            return ERR_INVALID, lambda: ws.move(one, cost_old=co) if arg % 2 else ws.move(one, cost_new=co)
        if kind == "move_stride":
            return ERR_INVALID, lambda: ws.move(one, cost_old=co, cost_new=co + 1.0, stride=ws.max_labels - 1)
    raise KeyError(kind)


def apply(side, sh, step):
    """applies one step to ``side.t``; returns what an observing step saw (None otherwise).  ``sh``: the shadow of the session — its
    MODEL is read where a step's arguments are made from the current costs (the same for every side)"""
    op, a = step
    t = side.t
    if op == "upload":
        key, cost_seed, prec, ro_seed, refused_first = a
        m = model_with_costs(key, cost_seed, strict=prec == "f32")
        if refused_first:
            ok, got = _expect(ERR_UNSUPPORTED, lambda: t.upload(m, rows_layout=True, table_precision="f32_round"))
            if not ok:
                raise Mismatch("upload with float tables under the rows layout: expected LPMP_ERR_UNSUPPORTED, got " + got)
            ok, got = _expect(ERR_STATE, t.lower_bound)
            if not ok:
                raise Mismatch("after a refused upload the engine holds no model: expected LPMP_ERR_STATE, got " + got)
        if side.ids:
            side.stale_id = sorted(side.ids.values())[0]
        side.ids = {}
        _upload(side, m, prec, props(key)["rows_layout"])
        for r in side.old_readouts or ():
            r.close()
        side.old_readouts = side.readouts
        sub, _ = vector_subset(m, ro_seed)
        side.readouts = (t.readout(sub), t.readout(None))
        for w in side.old_wsets:
            w.close()
        side.old_wsets, side.wsets = [side.wsets[k] for k in sorted(side.wsets)], {}
        for _, w in side.old_psets:
            w.close()
        side.old_psets, side.psets = [side.psets[k] for k in sorted(side.psets)], {}
    elif op == "window_set_create":
        side.wsets[a[0]] = t.window_set(window_list(sh.raw, a[1]))
    elif op == "window_set_destroy":
        side.wsets.pop(a[0]).close()
    elif op == "move_windows":
        ws = side.wsets[a[0]]
        _, delta, co, cn, stride = move_args(sh.raw, sh.nominal, sh.window_lists[a[0]], a[1], a[2], a[3])
        if a[2].startswith("device") and isinstance(t, E.Engine):
            import torch
            td = torch.from_numpy(delta.astype(np.int32)).cuda()
            tc = None if co is None else (torch.from_numpy(co).cuda(), torch.from_numpy(cn).cuda())
            torch.cuda.synchronize()
            if tc is None:
                ws.move(delta_dev=td.data_ptr())
            else:
                ws.move(delta_dev=td.data_ptr(), cost_dev=(tc[0].data_ptr(), tc[1].data_ptr()), stride=stride)
            t.synchronize()                           # (the call is asynchronous: the arrays live until it has run)
        else:
            ws.move(delta, cost_old=co, cost_new=cn)
    elif op in ("path_set_create", "forest_set_create"):
        kind, groups = sh.set_lists[a[0]]
        side.psets[a[0]] = (kind, t.path_set(groups) if kind == "path" else t.forest_set(groups))
    elif op in ("path_set_destroy", "forest_set_destroy"):
        side.psets.pop(a[0])[1].close()
    elif op in ("path_moves", "forest_moves"):
        side.psets[a[0]][1].move(a[1])
    elif op == "upload_primal":
        t.upload_primal(primal_for(sh.raw, a[0], a[1]))
    elif op == "compute_pass_custom":
        t.compute_pass_custom(*custom_rows(_key_of(sh), a[0]))
    elif op == "schedule_create":
        side.ids[a[0]] = t.schedule_create(*custom_rows(_key_of(sh), a[1]), fuse=a[2])
    elif op in ("schedule_run", "schedule_destroy"):
        getattr(t, op)(side.ids[a[0]])
    elif op == "upload_costs_cold":
        new = _recost(sh, a[0])
        t.upload_costs(const=new.const_data, duals=new.dual_data)
    elif op == "upload_costs_warm":
        t.upload_costs(const=_recost(sh, a[0]).const_data)           # constants only: the messages and the unaries stay
    elif op == "set_vectors_diff":
        # the second half of the header's warm start: on the changed unaries the difference new - old, accumulated
        new, old = sh.warm_new, sh.nominal
        v = vectors_of(sh.raw)
        doff, L = sh.raw.dual_offsets(), int(sh.raw.f_dim0[v].max())
        diff = np.zeros((len(v), L))
        for i, f in enumerate(v):
            n = int(sh.raw.f_dim0[f])
            diff[i, :n] = new[doff[f]:doff[f] + n] - old[doff[f]:doff[f] + n]
        t.set_vectors(v, diff, accumulate=True)
    elif op == "set_vectors":
        f, rows = vector_subset(sh.raw, a[0])
        t.set_vectors(f, rows, accumulate=a[1])
    elif op == "set_constants":
        f = RP.listed_subset_shift(sh.raw, a[0])            # (DIFF_SHIFT factors listed, too: rows {scale, integer shift})
        t.set_constants(f, RP.rows_for_shift(sh.raw, f, a[0], float_valued=sh.prec == "f32"))
    elif op == "upload_shared_pool":
        t.upload_shared_pool(pool_variant(sh.raw, a[0]))
    elif op == "upload_duals":
        t.upload_duals(sh.pending_duals)
    elif op == "refused":
        if (a[0] == "stale_readout" and side.old_readouts is None) or (a[0] == "stale_schedule" and side.stale_id is None):
            return None                                   # (an engine that took over in the middle of a replay has no older handles)
        if a[0] == "stale_window_set" and not side.old_wsets:
            return None
        if a[0] in ("stale_path_set", "stale_forest_set") and not [1 for k, _ in side.old_psets if k == a[0].split("_")[1]]:
            return None
        code, call = _refused(side, sh, a[0], a[1])
        ok, got = _expect(code, call)
        if not ok:
            raise Mismatch("refusal %s: expected %s, got %s" % (a[0], code, got))
        if a[0] == "stale_window_set":
            side.old_wsets.pop(0).close()                 # destroying it stays legal
        if a[0] in ("stale_path_set", "stale_forest_set"):
            k = [k for k, _ in side.old_psets].index(a[0].split("_")[1])
            side.old_psets.pop(k)[1].close()              # destroying it stays legal
    elif op == "labels":
        if sh.labels is not None and sh.labels.min() < 0:
            # a stray negative label (upload_primal, form stray) that no move has replaced yet: the array is compared; its cost and its
            # consistency are outside the contract of lpmp_evaluate_primal and are not asked for
            return (None, None, t.download_primal())
        return (t.evaluate_primal(), t.check_primal_consistency(), t.download_primal())
    elif op in ("ro_labels", "ro_vectors", "ro_beliefs"):
        return tuple(getattr(r, op[3:])() for r in side.readouts)
    elif op in ("lower_bound", "factor_lower_bounds", "download_duals"):
        return getattr(t, op)()
    else:
        getattr(t, op)(*a)
    return None


def _key_of(sh):
    return sh.key


def _recost(sh, seed):
    return model_with_costs(sh.key, seed, sh.prec == "f32")


def _first_diff(x, y):
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape:
        return "shapes %s / %s" % (x.shape, y.shape)
    bad = np.argwhere(~((x == y) | (_nan(x) & _nan(y))))
    i = tuple(int(k) for k in bad[0])
    return "first difference at %s: %r / %r (%d entries differ)" % (i, x[i].item(), y[i].item(), len(bad))


def _nan(x):
    return np.isnan(x) if x.dtype.kind == "f" else np.zeros(x.shape, bool)


def compare(op, got, want, pair=False):
    """None, or what differs between an observation and the shadow's (``pair``: between two engines, where a tracked and a recomputed
    bound may differ in the last bit: tests/test_speculation_gpu.py lines 115-121)"""
    if op == "lower_bound":
        tol = PAIR_TOL * (1.0 + abs(want)) if pair else LB_RTOL * max(1.0, abs(want))
        return None if np.isfinite(got) and abs(got - want) <= tol else "lower bound %r / %r" % (got, want)
    if op == "factor_lower_bounds":
        tol = PAIR_TOL * (1.0 + np.abs(want)) if pair else FLB_ATOL
        return None if got.shape == want.shape and np.all(np.abs(got - want) <= tol) else "factor bounds: " + _first_diff(got, want)
    if op == "download_duals":
        return None if np.array_equal(got, want) else "duals: " + _first_diff(got, want)
    if op == "labels":
        (c, ok, lab), (cw, okw, labw) = got, want
        if not np.array_equal(lab, labw):
            return "labels: " + _first_diff(lab, labw)
        if ok != okw:
            return "check_primal_consistency %r / %r" % (ok, okw)
        if c is None and cw is None:
            return None
        if pair or np.isinf(cw) or np.isinf(c):
            return None if c == cw else "evaluate_primal %r / %r" % (c, cw)
        # tests/test_decode_gpu.py test_decoded_labels_are_consistent_and_cost_the_original_energy: abs(cost - want) <= 1e-9 * max(1, abs(want))
        return None if abs(c - cw) <= ENERGY_RTOL * max(1.0, abs(cw)) else "evaluate_primal %r / %r" % (c, cw)
    # read-outs: tests/test_readout_gpu.py _check_labels_vectors (lines 91-92) and _check_beliefs (line 69): np.array_equal, equal_nan
    for k, (x, y) in enumerate(zip(got, want)):
        same = np.array_equal(x, y, equal_nan=True) if np.asarray(x).dtype.kind == "f" else np.array_equal(x, y)
        if not same:
            return "%s of read-out %d: %s" % (op, k, _first_diff(x, y))
    return None


def run(engines, shadow, session, observe=None, cell="?", seed="?", borrowed=False, reach=None, fresh_at=None, fresh=None, log=None, skip=None):
    """applies every step to every engine of ``engines`` (one, or two for the pair tests) and to ``shadow``, and compares: an observing
    step at once, the duals after a state-changing step where ``observe`` (``observe_plan(cell, seed, session)``; None: always) says so —
    about one step in four, since a download settles a speculative batch —, everything after the last step.  The first mismatch raises ``Mismatch``.
    ``fresh_at`` / ``fresh``: at that step a new engine (made by ``fresh()``) takes over with the shadow's model and duals.
    ``skip``: {engine number: ops it is not given} — knobs only, for the engine of a pair that keeps a setting."""
    skip = skip or {}
    engines = list(engines) if isinstance(engines, (list, tuple)) else [engines]
    sides = [_Side(e, borrowed) for e in engines]
    ssh = _Side(shadow)
    reach = reach if reach is not None else Reach()

    def fail(i, what):
        lines = ["session %s seed %s, step %d %s%r: %s" % (cell, seed, i, session[i][0], session[i][1], what), "the last steps:"]
        lines += ["  %3d %s%r" % (k, session[k][0], session[k][1]) for k in range(max(0, i - 7), i + 1)]
        ex = Mismatch("\n".join(lines))
        ex.index = i
        return ex

    def check(i, op):
        try:
            want = apply(ssh, shadow, (op, ()))
            seen = [apply(s, shadow, (op, ())) for s in sides]
        except E.EngineError as ex:
            if ex.code == ERR_DEVICE:
                raise
            raise fail(i, "%s raised EngineError %s: %s" % (op, ex.code, ex))
        for got in seen:
            if op == "lower_bound" and np.isfinite(got):      # (what the tracked sum differs by from the oracle's: printed with the reach)
                reach.lb_rel_max = max(reach.lb_rel_max, abs(got - want) / max(1.0, abs(want)))
            bad = compare(op, got, want)
            if bad:
                raise fail(i, bad + "  (engine / shadow)")
        if len(seen) == 2:
            bad = compare(op, seen[0], seen[1], pair=True)
            if bad:
                raise fail(i, bad + "  (first / second engine)")

    try:
        for i, (op, a) in enumerate(session):
            if log:
                log(i, op, a)
            cls = OP_CLASS[op]
            if fresh_at is not None and i == fresh_at:
                d = shadow.download_duals()
                for s in sides:
                    s.close(); s.t.close()
                    s.t = fresh()
                    _upload(s, RP.with_duals(shadow.raw, d), shadow.prec, props(shadow.key)["rows_layout"])
                    s.t.set_reparametrization_type(shadow.rtype)
                    if shadow.mode is not None:
                        s.t.set_reparametrization(shadow.mode)
                    s.readouts = tuple(s.t.readout(None if r is None else r) for r in shadow.ro_lists)
                    s.ids = {slot: s.t.schedule_create(*rows) for slot, rows in shadow.slot_rows.items()}
                    s.wsets = {slot: s.t.window_set(lst) for slot, lst in shadow.window_lists.items()}
                    s.psets = {slot: (k, s.t.path_set(g) if k == "path" else s.t.forest_set(g)) for slot, (k, g) in shadow.set_lists.items()}
                    if props(shadow.key)["mrf"]:                    # the labels, too: a later labels / read-out step compares them
                        s.t.upload_primal(shadow.download_primal())
                engines[:] = [s.t for s in sides]
            if cls in OBSERVING:
                check(i, op)
                continue
            if op == "upload":
                shadow.key, shadow.slot_rows, shadow.window_lists, shadow.warm_new = a[0], {}, {}, None
                shadow.set_lists, shadow.sets_at_window_move = {}, set()
                shadow.ro_lists = (vector_subset(base_model(a[0]), a[3])[0], None)
            if op in ("path_set_create", "forest_set_create"):
                shadow.set_lists[a[0]] = ("path", path_list(shadow.key, a[1])) if op[0] == "p" else ("forest", forest_list(shadow.key, a[1]))
            if op in ("path_set_destroy", "forest_set_destroy"):
                shadow.set_lists.pop(a[0], None)
            if op == "move_windows":
                shadow.sets_at_window_move = set(shadow.set_lists)
            if op == "window_set_create":
                shadow.window_lists[a[0]] = window_list(shadow.raw, a[1])
            if op == "window_set_destroy":
                shadow.window_lists.pop(a[0], None)
            if op == "move_windows":                               # what the shadow keeps of the costs follows the move (below)
                mf, md, _, mcn, _ = move_args(shadow.raw, shadow.nominal, shadow.window_lists[a[0]], a[1], a[2], a[3])
            if op == "upload_duals":
                shadow.pending_duals = shadow.download_duals() * 0.5
            if op == "schedule_create":
                shadow.slot_rows[a[0]] = custom_rows(shadow.key, a[1]) + (a[2],)
            if op == "schedule_destroy":
                shadow.slot_rows.pop(a[0], None)
            try:
                for k, s in enumerate(sides):
                    if op in skip.get(k, ()):
                        continue
                    if op == "reset_kernel_timing" and isinstance(s.t, E.Engine):
                        reach.before_reset(s.t)
                    counted = ("move_windows", "window_set_create", "path_moves", "forest_moves", "path_set_create", "forest_set_create")
                    built = s.t.schedules_built() if op in counted and isinstance(s.t, E.Engine) else None
                    apply(s, shadow, (op, a))
                    if built is not None and OP_CLASS[op] in ("relabel", "sets"):
                        # lpmp_path_set_create / lpmp_forest_set_create: "lpmp_schedules_built counts the create ONCE; a move plans and
                        # uploads nothing"
                        reach.path_moves += op == "path_moves"
                        reach.forest_moves += op == "forest_moves"
                        reach.move_sets += op.endswith("_create")
                        if op.endswith("_moves"):
                            un = shadow.raw.f_kind == M.F_VECTOR
                            reach.moves_on_unset += bool(np.all(shadow.labels[un, 0] >= shadow.raw.f_dim0[un]))
                            reach.moves_behind_windows += a[0] in shadow.sets_at_window_move
                        if s.t.schedules_built() != built + op.endswith("_create"):
                            raise Mismatch("schedules_built went from %d to %d" % (built, s.t.schedules_built()))
                    elif built is not None:
                        # lpmp_window_set_create: "counted ONCE by lpmp_schedules_built"; lpmp_move_windows: "plans nothing"
                        reach.moves += op == "move_windows"
                        reach.window_sets += op == "window_set_create"
                        if s.t.schedules_built() != built + (op == "window_set_create"):
                            raise Mismatch("schedules_built went from %d to %d" % (built, s.t.schedules_built()))
                apply(ssh, shadow, (op, a))
            except Mismatch as ex:
                raise fail(i, str(ex))
            except E.EngineError as ex:
                if ex.code == ERR_DEVICE:                           # a device error is no mismatch: the caller stops using the device
                    raise
                raise fail(i, "a call the step did not announce as refused raised EngineError %s: %s" % (ex.code, ex))
            if op in ("upload", "upload_costs_cold"):
                shadow.nominal = shadow.raw.dual_data if op == "upload" else _recost(shadow, a[0]).dual_data
            if op == "upload_costs_warm":
                shadow.warm_new = _recost(shadow, a[0]).dual_data
            if op == "set_vectors_diff":
                shadow.nominal = shadow.warm_new
            if op == "move_windows":
                for s in sides:                                     # a borrowed constants buffer: the packed shifts, bit for bit
                    if s.keep is not None:
                        s.t.synchronize()
                        got = s.keep[0].cpu().numpy()
                        if got.tobytes() != np.ascontiguousarray(shadow.raw.const_data, np.float64).tobytes():
                            raise fail(i, "packed constants in the caller's buffer: " + _first_diff(got, shadow.raw.const_data))
                shadow.nominal = moved_nominal(shadow.raw, shadow.nominal, mf, md, mcn)
                if getattr(shadow, "warm_new", None) is not None:
                    shadow.warm_new = moved_nominal(shadow.raw, shadow.warm_new, mf, md)
            for s in sides:
                if isinstance(s.t, E.Engine):
                    reach.after_step(s.t, op, a, shadow.mode)
            if observe is None or observe[i]:
                check(i, "download_duals")
            if cls == "refused":                                   # the point of a refusal is the state after it
                check(i, "factor_lower_bounds")
        last = len(session) - 1
        for op in ("download_duals", "lower_bound", "factor_lower_bounds", "ro_labels", "ro_vectors") + (("labels", "ro_beliefs") if props(shadow.key)["mrf"] else ()):
            check(last, op)
        for s in sides:
            if isinstance(s.t, E.Engine):
                reach.before_reset(s.t)
    finally:
        for s in sides + [ssh]:
            s.close()
    return reach
