"""Prepared read-outs, host side: the numpy statement of the belief rule (tests/readout_cases.py) pinned against the
CPU oracle — a unary that receives over all its messages and sends nothing ends with exactly the belief, in the order of its
message list and not in ascending message index —, and the ABI.  No GPU."""
import os
import re

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from oracle.binding import Oracle

import readout_cases as R

ANISO = M.REPAM_ANISOTROPIC
NEW = ("lpmp_readout_create", "lpmp_readout_labels", "lpmp_readout_vectors", "lpmp_readout_beliefs")

GRID_CASES = [(L, kind) for L in (3, 7) for kind in ("dense", "potts", "shared", "diff")]


def _dense(m):
    """the model the oracle runs: SHARED / DIFF factors as the DENSE factors they are bit for bit"""
    return m.expand_shared().expand_diff()


def _receive_all(m, passes=2):
    """(duals after ``passes`` anisotropic passes of the oracle, {u: theta_u after u alone received over all its messages and sent
    nothing from those duals})"""
    o = Oracle(_dense(m))
    o.set_reparametrization(ANISO)
    o.ComputePass(passes)
    duals = o.duals()
    doff = m.dual_offsets()
    off, _ = o.msg_lists()
    out = {}
    for u in R.unaries(m):
        k = int(off[u + 1] - off[u])
        o.set_duals(duals)
        o.compute_pass_custom([u], [0, k], np.zeros(k), [0, k], np.ones(k, np.uint8))
        out[u] = o.duals()[doff[u]:doff[u + 1]].copy()
    return duals, out


def _differing_rows(m, order):
    duals, want = _receive_all(m)
    got = R.beliefs_np(m, duals, order=order)
    us = R.unaries(m)
    return [u for i, u in enumerate(us) if not np.array_equal(got[i, :len(want[u])], want[u])]


@pytest.mark.parametrize("L,kind", GRID_CASES)
def test_statement_equals_the_oracles_receive_phase(L, kind):
    m = R.grid(4, 5, L, kind)
    assert _differing_rows(m, "list") == []


def test_ascending_message_index_is_another_order():
    """the guard of the order: with the messages taken in ascending index at least one of the eight grids differs from the oracle
    in the last bits (and the two orders do differ: the first unary of a grid receives over messages [2, 0])"""
    lists = R.message_lists(R.grid(4, 5, 3))
    assert lists[0] == [2, 0]
    differing = [(L, kind) for L, kind in GRID_CASES if _differing_rows(R.grid(4, 5, L, kind), "index")]
    print("grids on which ascending message index differs from the oracle:", differing)
    assert len(differing) >= 1


def test_rectangular_chain_both_sides():
    m = R.rect_chain()
    sides = {(int(m.f_dim0[int(m.m_left[k])]), int(m.mtypes[int(m.m_type[k])].param)) for k in range(m.n_messages)}
    assert sides == {(4, 0), (7, 1)} and int(m.f_dim0[1]) != int(m.f_dim0[0])
    assert _differing_rows(m, "list") == []


def test_float_tables():
    m = R.grid(4, 5, 7).with_f32_tables()
    assert not np.array_equal(m.const_data, R.grid(4, 5, 7).const_data)
    assert _differing_rows(m, "list") == []


def test_padding_is_nan_and_lists_are_free():
    m = R.ragged()
    duals = m.dual_data
    us = [2, 0, 2, 1]
    b = R.beliefs_np(m, duals, us, stride=36)
    assert b.shape == (4, 36) and np.array_equal(b[0], b[2], equal_nan=True)
    for i, u in enumerate(us):
        d = int(m.f_dim0[u])
        assert not np.isnan(b[i, :d]).any() and np.isnan(b[i, d:]).all()


def test_abi_declares_and_exports_the_calls():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "lpmp_engine.h")).read()
    L = E.lib()
    for fn in NEW:
        assert re.search(r"\bint %s\(" % fn, hdr) and fn in E.EXPORTS and hasattr(L, fn)
    for fn in ("lpmp_readout_destroy", "lpmp_readout_n", "lpmp_readout_max_labels"):
        assert fn in hdr and fn in E.EXPORTS and hasattr(L, fn)
    assert hasattr(E.Engine, "readout") and hasattr(E.Readout, "beliefs")
