"""Prepared read-outs (lpmp_readout_*): the numpy statement of the belief rule and the models of
tests/test_readout_host.py and tests/test_readout_gpu.py.  Written from the rule as include/lpmp_engine.h states it, not from the
device code.  Models are built once per process and never modified."""
import dataclasses
import functools

import numpy as np

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

import decode_cases as DC

INF = float("inf")


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def cost_table(m, coff, p):
    """cost_p as a [d0, d1] array: the pairwise cost of include/lpmp_model.h (DENSE: the table; POTTS: a == b ? 0.0 : diff;
    SHARED / DIFF / DIFF_SHIFT: ONE multiply scale * entry)"""
    kind, d0, d1 = int(m.f_kind[p]), int(m.f_dim0[p]), int(m.f_dim1[p])
    c = int(coff[p])
    if kind == M.F_PAIRWISE_DENSE:
        return m.const_data[c:c + d0 * d1].reshape(d0, d1)
    if kind == M.F_PAIRWISE_POTTS:
        return np.where(np.eye(d0, dtype=bool), 0.0, np.float64(m.const_data[c]))
    scale = np.float64(m.const_data[c])
    t = int(m.f_table[p])
    if kind == M.F_PAIRWISE_SHARED:
        return scale * m.shared_table(t)
    if kind == M.F_PAIRWISE_DIFF_SHIFT:      # scale * D[clip(a - b + shift, 0, n - 1)], the shift converted as the device converts it
        n, s = int(m.sh_dim1[t]), M.diff_shift_int(m.const_data[c + 1])
        D = m.sh_data[int(m.sh_off[t]): int(m.sh_off[t]) + n]
        return scale * D[np.clip(np.arange(d0)[:, None] - np.arange(d1)[None, :] + s, 0, n - 1)]
    assert kind == M.F_PAIRWISE_DIFF
    D = m.sh_data[int(m.sh_off[t]): int(m.sh_off[t]) + d0 + d1 - 1]
    return scale * D[np.arange(d0)[:, None] - np.arange(d1)[None, :] + (d1 - 1)]


def message_lists(m):
    """per factor the messages it is the LEFT factor of, in the order of its message list (lpmp_plan_get_msg_lists: the order in
    which a sweep receives); asserts that a vector factor has no others"""
    off, ent = E.Plan(m).msg_lists(m.n_messages)
    out = []
    for f in range(m.n_factors):
        e = ent[off[f]:off[f + 1]]
        if m.f_kind[f] == M.F_VECTOR:
            assert np.all(e % 2 == 0), f
        out.append([int(k) // 2 for k in e if k % 2 == 0])
    return out


def belief_row(m, duals, u, msgs, doff, coff):
    """b of unary u over the messages ``msgs`` in that order"""
    d0 = int(m.f_dim0[u])
    b = np.array(duals[doff[u]:doff[u] + d0], np.float64)
    for k in msgs:
        mt = m.mtypes[int(m.m_type[k])]
        assert mt.kind == M.M_UNARY_PAIRWISE and int(m.m_left[k]) == u
        p, s = int(m.m_right[k]), int(mt.param)
        p0, p1 = int(m.f_dim0[p]), int(m.f_dim1[p])
        T = cost_table(m, coff, p)
        m0, m1 = duals[doff[p]:doff[p] + p0], duals[doff[p] + p0:doff[p] + p0 + p1]
        if s == 0:
            q = (T + m1[None, :]).min(axis=1)
            ms = m0
        else:
            q = (T + m0[:, None]).min(axis=0)
            ms = m1
        assert q.shape == (d0,)
        b = b + (ms + q)
    return b


def beliefs_np(m, duals, factors=None, stride=None, order="list"):
    """[n, stride] float64, NaN beyond a factor's label count: row i is the belief of ``factors[i]`` (None: every VECTOR factor in
    ascending index) on the packed ``duals``.  ``order``: "list" — the rule: the order of the factor's message list — or "index":
    ascending message index, which is NOT the rule (tests/test_readout_host.py shows that the two differ in the last bits)"""
    duals = np.asarray(duals, np.float64)
    if factors is None:
        factors = [f for f in range(m.n_factors) if m.f_kind[f] == M.F_VECTOR]
    factors = [int(f) for f in factors]
    lists = message_lists(m)
    doff, coff = m.dual_offsets(), m.const_offsets()
    width = max([int(m.f_dim0[f]) for f in factors], default=0)
    stride = width if stride is None else stride
    out = np.full((len(factors), stride), np.nan)
    for i, u in enumerate(factors):
        msgs = lists[u] if order == "list" else sorted(lists[u])
        out[i, :int(m.f_dim0[u])] = belief_row(m, duals, u, msgs, doff, coff)
    return out


def vectors_np(m, duals, factors, stride=None):
    doff = m.dual_offsets()
    width = max([int(m.f_dim0[f]) for f in factors], default=0)
    stride = width if stride is None else stride
    out = np.full((len(factors), stride), np.nan)
    for i, u in enumerate(factors):
        out[i, :int(m.f_dim0[u])] = duals[doff[u]:doff[u] + int(m.f_dim0[u])]
    return out


def unaries(m):
    return [f for f in range(m.n_factors) if m.f_kind[f] == M.F_VECTOR]


# ---- models --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid(H, W, L, pairwise="dense", order="row_major", seed=1):
    return S.grid_model(H, W, L, pairwise=pairwise, order=order, seed=seed)


@functools.lru_cache(maxsize=None)
def ragged():
    """label counts 2, 5 and 33 (lane groups of two widths and a wave) around rectangular tables"""
    r = np.random.default_rng(17)
    dims = [2, 5, 33, 5, 2, 33]
    un = [r.random(d) for d in dims]
    pairs = [(0, 1), (1, 2), (2, 3), (4, 3), (5, 4), (0, 5), (2, 5)]
    return DC.build_model(un, [(i, j, ("dense", r.random((dims[i], dims[j])))) for i, j in pairs])


@functools.lru_cache(maxsize=None)
def rect_chain(d0=4, d1=7):
    """a chain over variables of d0, d1, d0, d1 labels: rectangular tables with the inner variables on either side"""
    r = np.random.default_rng(23)
    un = [r.random(d0), r.random(d1), r.random(d0), r.random(d1)]
    return DC.build_model(un, [(0, 1, ("dense", r.random((d0, d1)))), (2, 1, ("dense", r.random((d0, d1)))), (2, 3, ("dense", r.random((d0, d1))))])


@functools.lru_cache(maxsize=None)
def hub(n_leaves=9, L=5):
    return DC.star(n_leaves=n_leaves, L=L, seed=12)


@functools.lru_cache(maxsize=None)
def inf_row_pair(L=7):
    """(finite, with_inf_row): the graph of decode_cases.inf_tables_case with scattered +inf entries; in the second model row 2 of the
    first table (factor ``inf_row_factor``) is +inf as a whole.  An all-+inf row turns duals into NaN within one pass (the receive
    leaves -inf in the pairwise vector, the send adds +inf to it) and NaN is outside the contract of the read-out, so the duals this
    case is read on are those of two passes on the first model."""
    a = DC.inf_tables_case()
    assert int(a.f_dim0[0]) == L
    p = inf_row_factor(a)
    coff = a.const_offsets()
    const = a.const_data.copy()
    const[coff[p] + 2 * L: coff[p] + 3 * L] = INF
    return a, dataclasses.replace(a, const_data=const, _keep=[])


def inf_row_factor(m):
    return int(np.flatnonzero(m.f_kind == M.F_PAIRWISE_DENSE)[0])


@functools.lru_cache(maxsize=None)
def labeling_model():
    """vector factors joined by labeling / min-norm messages (no unary-pairwise structure)"""
    return S.multicut_triangle_model(6, 4, seed=1)
