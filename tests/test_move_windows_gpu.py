"""lpmp_move_windows on the device: label windows that move, with the duals and the shifts carried along.  After two passes (no dual
is trivial) the windows move; the duals are compared with ``np.array_equal`` against ``lp_mp_amd.model.move_windows``, the numpy
statement of the rule, and two more passes against the CPU oracle on ``expand_diff()`` of the moved model — duals bit for bit, the
lower bound within 1e-5 relative, as in tests/test_diff_shift_gpu.py.  Where the constants live in a buffer of the test's own the
packed scalars are read back and compared bit for bit, too."""
import numpy as np
import pytest
import torch

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from oracle.binding import Oracle

import move_windows_cases as C

pytestmark = pytest.mark.gpu

LB_RTOL = 1e-5
ANISO, UNIFORM = M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM
INVALID, UNSUPPORTED, STATE = -1, -2, -4


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def _oracle(m2, d2, mode):
    o = Oracle(C.D.with_duals(C.expand(m2), d2))
    o.set_reparametrization(mode)
    return o


def _close(a, b):
    return np.isfinite(a) and abs(a - b) <= LB_RTOL * max(1.0, abs(b))


def _start(eng, m, mode, passes=2, **kw):
    eng.upload(m, **kw)
    eng.set_reparametrization(mode)
    eng.compute_pass(passes)
    return eng.download_duals()


def _move_and_check(eng, m, lst, delta, mode=ANISO, cost_old=None, cost_new=None, passes=2):
    """two passes, the move, the duals against the numpy statement, the bound and ``passes`` more passes against the oracle on the
    dense expansion of the moved model; returns (moved model, moved duals)"""
    d = _start(eng, m, mode)
    ws = eng.window_set(lst)
    built = eng.schedules_built()
    ws.move(delta, cost_old=cost_old, cost_new=cost_new)
    assert eng.schedules_built() == built                  # a move plans and builds nothing
    m2, d2 = M.move_windows(m, d, lst, delta, cost_old, cost_new)
    got = eng.download_duals()
    assert not np.any(np.isnan(got)) and np.array_equal(got, d2), int(np.sum(got != d2))
    o = _oracle(m2, d2, mode)
    assert _close(eng.lower_bound(), o.LowerBound()), (eng.lower_bound(), o.LowerBound())
    eng.compute_pass(passes); o.ComputePass(passes)
    got = eng.download_duals()
    assert np.array_equal(got, o.duals()), float(np.max(np.abs(got - o.duals())))
    assert _close(eng.lower_bound(), o.LowerBound()), (eng.lower_bound(), o.LowerBound())
    ws.close()
    return m2, d2


@pytest.mark.parametrize("L", C.GRID_LABELS)
@pytest.mark.parametrize("order", C.ORDERS)
def test_grids(eng, L, order):
    """6 x 5 grids, vectors of the lengths 1, 2, 5, L, 2L - 1, 3L; a delta per unary from 0, +-1, +-63, +-64, +-(L - 1), +-L, +-(L + 7)
    and random values — from 130 labels on with both signs of 64 <= |delta| < L, the in-place hazard"""
    m = C.grid(L, order)
    u = C.unaries(m)
    assert sorted(set(m.sh_dim1)) == sorted(set(C.D.vector_lengths(L)))
    delta = C.deltas(m.f_dim0[u], L)
    assert {0, 1, -1, 63, -64, L - 1, -L, L + 7} <= set(delta.tolist())
    assert C.has_hazard(m.f_dim0[u], delta) or L < 130
    for mode in ((ANISO, UNIFORM) if L in (5, 130) else (ANISO,)):
        _move_and_check(eng, m, None if mode == ANISO else u, delta, mode)
    # listed in another order, with other moves: a row of delta belongs to its entry of the list
    lst = u[::-1]
    _move_and_check(eng, m, lst, C.deltas(m.f_dim0[lst], L + 1)[::-1].copy(), ANISO, passes=1)


@pytest.mark.parametrize("dims", C.RECT_DIMS)
def test_rectangular_chain(eng, dims):
    """unaries of two label counts on both sides of da x db and db x da factors"""
    m = C.D.rect_chain(dims=dims)
    u = C.unaries(m)
    assert set(m.f_dim0[u]) == set(dims)
    delta = C.deltas(m.f_dim0[u], 9)
    assert C.has_hazard(m.f_dim0[u], delta) or max(dims) < 130
    for mode in (ANISO, UNIFORM):
        _move_and_check(eng, m, u, delta, mode)
    _move_and_check(eng, m, u[1::2], delta[1::2], ANISO)       # only the unaries of the second label count


def _with_device_consts(eng, m, mode):
    """upload with the constants in a buffer of the test's own: the packed scalars a move writes can be read back"""
    t = torch.from_numpy(np.array(m.const_data, np.float64, copy=True)).cuda()
    torch.cuda.synchronize()
    eng.upload(m, const_dev=t.data_ptr(), keep=t)
    eng.set_reparametrization(mode)
    eng.compute_pass(2)
    return t, eng.download_duals()


def test_partly_listed_model(eng):
    """every second unary listed: unlisted vectors and the constants of factors with equal deltas are untouched, bit for bit"""
    m = C.grid(33, "colour_major")
    u = C.unaries(m)
    lst = u[::2]
    delta = np.where(np.arange(len(lst)) % 5 == 0, C.deltas(m.f_dim0[lst], 2), 4)      # most listed neighbours move alike
    t, d = _with_device_consts(eng, m, ANISO)
    ws = eng.window_set(lst)
    assert ws.n == len(lst) and ws.max_labels == 33 and ws.n_pairwise == E.Plan(m).window_info(lst)["n_pairwise"]
    ws.move(delta)
    m2, d2 = M.move_windows(m, d, lst, delta)
    got = eng.download_duals()
    assert got.tobytes() == d2.tobytes()
    off, coff = m.dual_offsets(), m.const_offsets()
    for f in u[1::2]:
        assert got[off[f]:off[f + 1]].tobytes() == d[off[f]:off[f + 1]].tobytes()
    const = t.cpu().numpy()
    assert const.tobytes() == m2.const_data.tobytes()
    _, links, pairs = M.window_links(m, lst)
    same = [p for p, l, r in pairs if (delta[l] if l >= 0 else 0) == (delta[r] if r >= 0 else 0)]
    moved = [p for p, l, r in pairs if (delta[l] if l >= 0 else 0) != (delta[r] if r >= 0 else 0)]
    assert moved and same and all(const[coff[p]:coff[p + 1]].tobytes() == m.const_data[coff[p]:coff[p + 1]].tobytes() for p in same)
    assert any(const[coff[p] + 1] != m.const_data[coff[p] + 1] for p in moved)
    o = _oracle(m2, d2, ANISO)
    eng.compute_pass(2); o.ComputePass(2)
    assert np.array_equal(eng.download_duals(), o.duals()) and _close(eng.lower_bound(), o.LowerBound())
    ws.close()


def test_equal_deltas_write_no_constant(eng):
    m = C.grid(5, "row_major")
    t, d = _with_device_consts(eng, m, ANISO)
    ws = eng.window_set()
    ws.move(np.full(ws.n, -2))
    m2, d2 = M.move_windows(m, d, None, np.full(ws.n, -2))
    assert eng.download_duals().tobytes() == d2.tobytes() and not np.array_equal(d2, d)
    assert t.cpu().numpy().tobytes() == m.const_data.tobytes() == m2.const_data.tobytes()
    ws.close()


def test_second_component_of_dense_factors(eng):
    """the DIFF_SHIFT grid's unaries move; a component of DENSE factors in the same model stays legal and unchanged"""
    m, u, other = C.two_component_model()
    with pytest.raises(E.EngineError) as ei:
        eng.upload(m); eng.window_set()
    assert ei.value.code == UNSUPPORTED and "factor %d " % other[0] in str(ei.value)
    lst = np.asarray(u[::2], np.int32)
    delta = np.array([3, -2, 0, 6, -7])
    d = _start(eng, m, ANISO)
    m2, d2 = _move_and_check(eng, m, lst, delta)
    off = m.dual_offsets()
    for f in other:
        assert d2[off[f]:off[f + 1]].tobytes() == d[off[f]:off[f + 1]].tobytes()


def test_inputs_from_device_memory(eng):
    """delta from device memory equals delta from the host; cost_old / cost_new from the host and from device pointers give the same
    result, with a stride above the longest vector"""
    m = C.grid(65, "colour_major")
    u = C.unaries(m)
    delta = C.deltas(m.f_dim0[u], 8)
    stride = 65 + 6
    co, cn = C.cost_pair(m, u, delta, 12, stride=stride, inf=True)
    out = []
    for dev in (False, True):
        d = _start(eng, m, ANISO)
        ws = eng.window_set(u)
        if dev:
            td = torch.from_numpy(np.concatenate([delta, [1 << 30]]).astype(np.int32)).cuda()
            to, tn = torch.from_numpy(co).cuda(), torch.from_numpy(cn).cuda()
            torch.cuda.synchronize()
            ws.move(delta_dev=td.data_ptr(), cost_dev=(to.data_ptr(), tn.data_ptr()), stride=stride)
            eng.synchronize()
            assert np.array_equal(td.cpu().numpy()[:-1], delta) and np.array_equal(to.cpu().numpy(), co, equal_nan=True)
        else:
            ws.move(delta, cost_old=co, cost_new=cn)
        out.append(eng.download_duals())
        ws.close()
    m2, d2 = M.move_windows(m, d, u, delta, co, cn)
    assert out[0].tobytes() == d2.tobytes() and out[1].tobytes() == d2.tobytes()
    o = _oracle(m2, d2, ANISO)
    eng.compute_pass(2); o.ComputePass(2)
    assert np.array_equal(eng.download_duals(), o.duals())
    # a device delta beyond +-2^20 is saturated where it is read: the move of a whole window either way
    d = _start(eng, m, ANISO)
    ws = eng.window_set(u[:2])
    td = torch.tensor([1 << 30, -(1 << 30)], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ws.move(delta_dev=td.data_ptr())
    m2, d2 = M.move_windows(m, d, u[:2], [M.MOVE_DELTA_MAX, -M.MOVE_DELTA_MAX])
    assert eng.download_duals().tobytes() == d2.tobytes()
    o = _oracle(m2, d2, ANISO)
    eng.compute_pass(1); o.ComputePass(1)
    assert np.array_equal(eng.download_duals(), o.duals())
    ws.close()


def test_zero_move(eng):
    m = C.grid(64, "row_major")
    ref = E.Engine(0)
    try:
        d0 = _start(ref, m, ANISO)
        d = _start(eng, m, ANISO)
        assert d.tobytes() == d0.tobytes()
        ws = eng.window_set()
        built = eng.schedules_built()
        ws.move(np.zeros(ws.n, np.int64))
        assert eng.schedules_built() == built
        assert eng.download_duals().tobytes() == d.tobytes()
        eng.compute_pass(2); ref.compute_pass(2)
        assert eng.download_duals().tobytes() == ref.download_duals().tobytes()
        assert eng.lower_bound() == ref.lower_bound()
        ws.close()
    finally:
        ref.close()


def test_create_counts_once_and_survives_new_costs(eng):
    m = C.grid(5, "colour_major")
    d = _start(eng, m, ANISO)
    built = eng.schedules_built()
    ws = eng.window_set()
    assert eng.schedules_built() == built + 1 and ws.n == 30 and ws.n_pairwise == C.D.n_edges(C.H, C.W)
    delta = C.deltas(m.f_dim0[C.unaries(m)], 1)
    ws.move(delta)
    m2, d2 = M.move_windows(m, d, None, delta)
    # the set is structure: new costs on the plan, then the same set moves again
    eng.upload_costs(const=m.const_data, duals=m.dual_data)
    eng.compute_pass(1)
    d = eng.download_duals()
    ws.move(-delta)
    m3, d3 = M.move_windows(m, d, None, -delta)
    assert eng.download_duals().tobytes() == d3.tobytes() and eng.schedules_built() == built + 1
    o = _oracle(m3, d3, ANISO)
    eng.compute_pass(2); o.ComputePass(2)
    assert np.array_equal(eng.download_duals(), o.duals())
    ws.close()


def test_state_after_a_move(eng):
    """labels unset, bound equal to the oracle's, a prepared schedule and a read-out made before the move still run"""
    m = C.D.primal_grid(16, "colour_major")
    u = C.unaries(m)
    eng.upload(m); eng.set_reparametrization(ANISO)
    eng.compute_pass(2)
    eng.decode_primal(0)
    assert np.isfinite(eng.evaluate_primal())
    plan = eng.plan
    fs = plan.update_order(0)
    (oo, om), (mo, mk) = plan.omega(0, ANISO), plan.mask(0, ANISO)
    sid = eng.schedule_create(fs, oo, om, mo, mk)
    r = eng.readout(u)
    d = eng.download_duals()
    ws = eng.window_set(u)
    delta = C.deltas(m.f_dim0[u], 6)
    ws.move(delta)
    assert eng.evaluate_primal() == np.inf
    assert np.array_equal(r.labels(), m.f_dim0[u])                     # unset: the label count
    m2, d2 = M.move_windows(m, d, u, delta)
    o = _oracle(m2, d2, ANISO)
    assert _close(eng.lower_bound(), o.LowerBound())
    off = m.dual_offsets()
    vec = r.vectors()
    for i, f in enumerate(u):
        assert np.array_equal(vec[i, :16], d2[off[f]:off[f] + 16])
    eng.schedule_run(sid)
    o.compute_pass_custom(fs, oo, om, mo, mk)
    assert np.array_equal(eng.download_duals(), o.duals()) and _close(eng.lower_bound(), o.LowerBound())
    eng.compute_pass_and_primal(2); o.ComputePassAndPrimal(2)
    assert np.array_equal(eng.download_primal(), o.primal())
    assert abs(eng.evaluate_primal() - o.EvaluatePrimal()) <= 1e-9 * max(1.0, abs(o.EvaluatePrimal()))
    eng.schedule_destroy(sid); r.close(); ws.close()


def test_move_inside_a_run_of_single_passes_with_speculation():
    """a move settles like every call that is not a plain pass: the result is that of the engine without speculation.  (Joined
    launches are one packed dense class today, so a model with DIFF_SHIFT factors opens no batch and the settling has nothing to
    roll back; the comparison holds whatever the engine decides to run ahead.)"""
    m = C.D.speculation_grid()
    u = C.unaries(m)
    delta = C.deltas(m.f_dim0[u], 3)
    out = []
    for depth in (0, 4):
        e = E.Engine(0)
        try:
            e.set_speculation(depth)
            e.upload(m); e.set_reparametrization(ANISO)
            ws = e.window_set(u)
            for _ in range(3):
                e.compute_pass(1)
            ws.move(delta)
            for _ in range(3):
                e.compute_pass(1)
            out.append((e.download_duals(), e.lower_bound()))
            ws.close()
        finally:
            e.close()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1] == out[1][1]


def test_state_error_while_the_constants_are_unspecified():
    """a refused lpmp_upload_costs (strict float tables) leaves the constants unspecified: a move would read a shift"""
    m, u, other = C.two_component_model()
    mf = m.with_f32_tables()
    assert not np.array_equal(mf.const_data, m.const_data)
    e = E.Engine(0)
    try:
        e.upload(mf, table_precision="f32"); e.set_reparametrization(ANISO)
        e.compute_pass(1)
        ws = e.window_set(u[::2])
        delta = np.array([1, -1, 2, 0, -3])
        with pytest.raises(E.EngineError) as ei:
            e.upload_costs(const=m.const_data)
        assert ei.value.code == UNSUPPORTED
        with pytest.raises(E.EngineError) as ei:
            ws.move(delta)
        assert ei.value.code == STATE and "constants are unspecified" in str(ei.value)
        e.upload_costs(const=mf.const_data)
        d = e.download_duals()
        ws.move(delta)
        m2, d2 = M.move_windows(mf, d, u[::2], delta)
        assert e.download_duals().tobytes() == d2.tobytes()
        o = _oracle(m2, d2, ANISO)
        e.compute_pass(1); o.ComputePass(1)
        assert np.array_equal(e.download_duals(), o.duals())
        ws.close()
    finally:
        e.close()


def test_refusals_of_the_call(eng):
    m = C.grid(5, "row_major")
    d = _start(eng, m, ANISO)
    ws = eng.window_set()
    L = eng.L
    delta = np.zeros(ws.n, np.int32); delta[7] = M.MOVE_DELTA_MAX + 1
    co = np.zeros((ws.n, 5))
    for call, code, what in (
            (lambda: ws.move(delta), INVALID, "entry 7"),
            (lambda: ws.move(-delta), INVALID, "entry 7"),
            (lambda: ws.move(np.zeros(ws.n, np.int32), cost_old=co), INVALID, "come together"),
            (lambda: ws.move(np.zeros(ws.n, np.int32), cost_new=co), INVALID, "come together"),
            (lambda: ws.move(np.zeros(ws.n, np.int32), cost_old=co, cost_new=co, stride=4), INVALID, "cost_stride 4"),
            (lambda: E._chk(L.lpmp_move_windows(eng.h, ws.h, None, 0, None, None, 0, 0)), INVALID, "null delta"),
            (lambda: E._chk(L.lpmp_move_windows(eng.h, ws.h, delta.ctypes.data, 2, None, None, 0, 0)), INVALID, "delta_mem")):
        with pytest.raises(E.EngineError) as ei:
            call()
        assert ei.value.code == code and what in str(ei.value), str(ei.value)
        assert eng.download_duals().tobytes() == d.tobytes()              # nothing was written
    with pytest.raises(ValueError):
        ws.move(np.zeros(ws.n - 1, np.int32))
    # refusals at create: the engine names what the plan names
    md, ud, pd, ed = C.edge_grid("dense")
    eng.upload(md)
    with pytest.raises(E.EngineError) as ei:                                # the set of the model that has been replaced
        ws.move(np.zeros(ws.n, np.int32))
    assert ei.value.code == STATE
    ws.close()                                                              # destroying it stays legal
    with pytest.raises(E.EngineError) as ei:
        eng.window_set()
    assert ei.value.code == UNSUPPORTED and "factor %d " % ud[ed[4][0]] in str(ei.value)
    with pytest.raises(E.EngineError) as ei:
        eng.window_set([ud[0], ud[0]])
    assert ei.value.code == INVALID and "listed twice" in str(ei.value)
    e2 = E.Engine(0)
    try:
        h = E.C.c_void_p()
        assert L.lpmp_window_set_create(e2.h, 0, None, E.C.addressof(h)) == STATE          # before an upload
    finally:
        e2.close()
    empty = eng.window_set([])
    empty.move([])
    assert empty.n == 0 and empty.n_pairwise == 0
    empty.close()
