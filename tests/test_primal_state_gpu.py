"""The primal state calls on the device: labels written into the primal array from host and device arrays
(lpmp_readout_set_labels), labels carried through a window move (lpmp_move_windows_carry) and the two scalars written into device
memory (lpmp_lower_bound_dev, lpmp_evaluate_primal_dev).  Every comparison is ``np.array_equal``, or the bits of a double: against
the numpy statements of tests/primal_state_cases.py and ``lp_mp_amd.model.move_labels``, against the host calls, and against a
twin engine that was given the same state through the calls that existed before."""
import numpy as np
import pytest
import torch

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

import diff_shift_cases as DS
import move_windows_cases as MW
import path_moves_cases as PM
import primal_state_cases as C
import test_bound_sum_gpu as BS

pytestmark = pytest.mark.gpu

ANISO = M.REPAM_ANISOTROPIC
NAN_BITS = 0x7FF8_0000_DEAD_BEEF                  # the sentinel around a destination: a NaN with a payload


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def twin():
    e = E.Engine(0)
    yield e
    e.close()


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


class Cell:
    """one double of device memory between two sentinels"""

    def __init__(self):
        self.t = _dev(np.full(3, NAN_BITS, np.uint64).view(np.float64))
        self.ptr = self.t.data_ptr() + 8

    def read(self, e):
        """the value, after the engine's stream has drained; the two neighbours must hold the sentinel's bits"""
        e.synchronize()
        h = self.t.cpu().numpy()
        assert _bits(h)[0] == NAN_BITS and _bits(h)[2] == NAN_BITS, [hex(int(b)) for b in _bits(h)]
        return h[1]


def _same(a, b):
    return _bits(a).tobytes() == _bits(b).tobytes()


def _refused(code, call, *names):
    with pytest.raises(E.EngineError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for n in names:
        assert n in str(ei.value), str(ei.value)


# ---- set_labels ------------------------------------------------------------------------------------------------------------------
LABEL_GRID = (17, 16, 5)                          # 272 unaries: read-outs of up to 257 rows


def _label_model():
    return PM.grid(*LABEL_GRID, "colour_major", pairwise="potts")


def _labels(m, f, seed):
    """a label per listed factor, every fifth the dimension (unset)"""
    r = np.random.default_rng(seed)
    src = r.integers(0, m.f_dim0[f]).astype(np.int32) if len(f) else np.zeros(0, np.int32)
    src[::5] = m.f_dim0[f][::5]
    return src


@pytest.mark.parametrize("n", C.READOUT_SIZES + (None,))
@pytest.mark.parametrize("source", ("host", "device"))
def test_set_labels_round_trip(eng, n, source):
    """a read-out of n unaries in a permuted order (None: ``factors=None``, all 272): the labels read back through
    lpmp_readout_labels and download_primal equal the input, unset values included; unlisted labels are untouched, the pairwise slots
    follow the unaries that hold a label, and the source array is unchanged"""
    m = _label_model()
    u = C.unaries(m)
    eng.upload(m)
    base = C.random_primal(m, 1, unset_every=7)
    eng.upload_primal(base)
    f = u if n is None else np.random.default_rng(n).permutation(u)[:n].astype(np.int32)
    r = eng.readout(None if n is None else f)
    assert r.n == len(f)
    src = _labels(m, f, 2)
    keep = src.copy()
    built = eng.schedules_built()
    if source == "host":
        r.set_labels(src)
        assert np.array_equal(src, keep)
    else:
        t = _dev(src if len(src) else np.zeros(1, np.int32))
        r.set_labels(src_dev=t.data_ptr())
        eng.synchronize()
        assert np.array_equal(t.cpu().numpy()[:len(src)], keep)
    assert eng.schedules_built() == built
    assert np.array_equal(r.labels(), keep)
    got = eng.download_primal()
    want = C.set_labels_reference(m, base, f, keep)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    rest = np.setdiff1d(u, f)
    assert np.array_equal(got[rest], base[rest])
    r.close()


def test_set_labels_first_use_makes_the_primal_array(eng):
    """no label call before it on this upload: the array is made as lpmp_readout_labels makes it, unlisted labels are unset"""
    m = _label_model()
    u = C.unaries(m)
    eng.upload(m)
    f = u[5:40]
    r = eng.readout(f)
    src = _labels(m, f, 3)
    r.set_labels(src_dev=_dev(src).data_ptr())
    got = eng.download_primal()
    assert np.array_equal(got, C.set_labels_reference(m, C.unset_primal(m), f, src))
    r.close()


def test_set_labels_refusals(eng):
    m = _label_model()
    u = C.unaries(m)
    d = int(m.f_dim0[u[0]])
    eng.upload(m)
    base = C.random_primal(m, 4)
    eng.upload_primal(base)
    f = u[:300:3].copy()
    r = eng.readout(f)
    good = _labels(m, f, 5)
    for bad, at in ((-1, 7), (d + 1, len(f) - 1)):
        src = good.copy()
        src[at] = bad
        _refused(C.INVALID, lambda: r.set_labels(src), "entry %d" % at, "factor %d" % f[at], "nothing was written")
        assert np.array_equal(eng.download_primal(), base)                    # nothing written
    # the same values from the device are stored as unset where they are read
    src = good.copy()
    src[7], src[-1], src[0], src[1] = -1, d + 1, -(1 << 31), (1 << 31) - 1
    r.set_labels(src_dev=_dev(src).data_ptr())
    want = src.copy()
    want[[7, -1, 0, 1]] = d
    assert np.array_equal(r.labels(), want)
    assert np.array_equal(eng.download_primal(), C.set_labels_reference(m, base, f, src))
    # a null source, a bad src_mem, a wrong number of labels
    assert eng.L.lpmp_readout_set_labels(eng.h, r.h, None, E.MEM_HOST) == C.INVALID
    assert eng.L.lpmp_readout_set_labels(eng.h, r.h, good.ctypes.data, 7) == C.INVALID
    with pytest.raises(ValueError):
        r.set_labels(good[:-1])
    # a read-out with a factor listed twice: refused for this call, its labels() still works
    before = eng.download_primal()
    dup = eng.readout(np.array([u[3], u[9], u[3], u[1]], np.int32))
    _refused(C.INVALID, lambda: dup.set_labels(np.zeros(4, np.int32)), "factor %d" % u[3], "twice")
    _refused(C.INVALID, lambda: dup.set_labels(src_dev=_dev(np.zeros(4, np.int32)).data_ptr()), "factor %d" % u[3])
    assert np.array_equal(dup.labels(), before[[u[3], u[9], u[3], u[1]], 0]) and np.array_equal(eng.download_primal(), before)
    # an empty read-out: a no-op after the checks, also with a null source
    empty = eng.readout(np.zeros(0, np.int32))
    empty.set_labels(np.zeros(0, np.int32))
    assert eng.L.lpmp_readout_set_labels(eng.h, empty.h, None, E.MEM_DEVICE) == 0
    assert eng.L.lpmp_readout_set_labels(eng.h, empty.h, None, 7) == C.INVALID
    assert np.array_equal(eng.download_primal(), before)
    # a read-out of a model replaced since
    eng.upload(m)
    _refused(C.STATE, lambda: r.set_labels(good), "another model")
    for x in (r, dup, empty):
        x.close()


def _defaults(*engines):
    """the module's engines go back to the default layout and table precision (both requests stay across uploads)"""
    for e in engines:
        e.upload(S.grid_model(3, 3, 2), rows_layout=False, table_precision="f64")


def _cost_model(kind):
    if kind == "diff_shift":
        return DS.shift_grid(6, 5, 9, order="colour_major", seed=4), {}
    if kind == "dense_f32":
        return S.grid_model(6, 5, 7, pairwise="dense", order="colour_major", seed=4), {"table_precision": "f32_round"}
    L = {"dense": 7, "potts": 6, "shared": 8, "diff": 11}[kind]
    return S.grid_model(6, 5, L, pairwise=kind, order="colour_major", seed=4), {}


@pytest.mark.parametrize("kind", C.COST_KINDS)
def test_cost_after_set_labels_equals_a_twin_after_upload_primal(eng, twin, kind):
    m, kw = _cost_model(kind)
    p = C.random_primal(m, 6)
    u = C.unaries(m)
    cell = Cell()
    try:
        for e in (eng, twin):
            e.upload(m, **kw)
            e.set_reparametrization(ANISO)
            e.compute_pass(2)
        r = eng.readout()
        r.set_labels(src_dev=_dev(p[u, 0].copy()).data_ptr())
        twin.upload_primal(p)
        a, b = eng.evaluate_primal(), twin.evaluate_primal()
        assert np.isfinite(b) and _same(a, b), (a, b)
        assert np.array_equal(eng.download_primal(), p)
        eng.evaluate_primal(cell.ptr)
        assert _same(cell.read(eng), b)
        r.close()
    finally:
        _defaults(eng, twin)


@pytest.mark.parametrize("source", ("host", "device"))
def test_path_moves_start_from_the_labels_set(eng, source):
    """path_moves after set_labels equals path_moves_reference started from those labels (9 x 7 grid, 8 labels)"""
    m = PM.grid(9, 7, 8, "colour_major")
    groups = S.grid_paths(9, 7, "colour_major")
    eng.upload(m)
    eng.set_reparametrization(ANISO)
    eng.compute_pass(2)
    duals = eng.download_duals()
    start = C.random_primal(m, 8)
    u = C.unaries(m)
    f = np.random.default_rng(9).permutation(u).astype(np.int32)
    r = eng.readout(f)
    src = start[f, 0].copy()
    if source == "host":
        r.set_labels(src)
    else:
        r.set_labels(src_dev=_dev(src).data_ptr())
    ps = eng.path_set(groups)
    ps.move(2)
    got = eng.download_primal()
    want = PM.path_moves_reference(m, duals, start, groups, rounds=2)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    assert not np.array_equal(got, start)
    ps.close(); r.close()


def test_set_labels_on_a_model_the_rounding_code_refuses(eng):
    """the Potts grid with labeling lists of the session `relabel_lists` cell: only the unary labels show (lpmp_download_primal is
    refused on such a model: the read-out of every VECTOR factor is the witness), and no call fails"""
    m, mg = C.lists_model()
    u = C.unaries(mg)
    every = C.unaries(m)
    eng.upload(m)
    eng.set_reparametrization(ANISO)
    eng.compute_pass(1)
    r, ra = eng.readout(u), eng.readout()
    want = C.unset_primal(m)
    for step, source in enumerate(("host", "device", "host")):
        src = _labels(m, u, 11 + step)
        if source == "host":
            r.set_labels(src)
        else:
            r.set_labels(src_dev=_dev(src).data_ptr())
        want = C.set_labels_reference(m, want, u, src, unaries_only=True)
        assert np.array_equal(r.labels(), src) and np.array_equal(ra.labels(), want[every, 0])
        if step == 0:
            cell = Cell()
            _refused(C.UNSUPPORTED, lambda: eng.evaluate_primal(cell.ptr))
            _refused(C.UNSUPPORTED, lambda: eng.evaluate_primal())
            assert np.array_equal(ra.labels(), want[every, 0])                # the refused calls left the array
    # path moves over the grid's rows and columns start from these labels, as on any model
    groups = S.grid_paths(5, 4, "colour_major")
    ps = eng.path_set(groups)
    ps.move(1)
    start = np.zeros((mg.n_factors, 2), np.int32)
    start[u, 0] = np.minimum(want[u, 0], mg.f_dim0[u] - 1)                    # (an unset neighbour is clamped where it is read)
    duals = eng.download_duals()[:mg.dual_data.shape[0]]
    ref = PM.path_moves_reference(mg, duals, PM.propagate(mg, start, PM.structure(mg)[1]), groups, rounds=1)
    assert np.array_equal(r.labels(), ref[u, 0])
    ps.close(); r.close(); ra.close()


# ---- move_windows_carry ----------------------------------------------------------------------------------------------------------
def _twins_after_passes(eng, twin, m):
    """both engines on ``m`` with the constants in buffers of the test's own (the shifts a move writes can be read back)"""
    bufs = []
    for e in (eng, twin):
        t = _dev(np.array(m.const_data, np.float64, copy=True))
        e.upload(m, const_dev=t.data_ptr(), keep=t)
        e.set_reparametrization(ANISO)
        e.compute_pass(2)
        bufs.append(t)
    return bufs


def _move(ws, delta, form, costs, carry):
    kw = dict(carry_labels=True) if carry else {}
    if costs is not None:
        kw.update(cost_old=costs[0], cost_new=costs[1])
    if form == "device_far":
        t = _dev(delta.astype(np.int32))
        ws.move(delta_dev=t.data_ptr(), **kw)
        return t
    ws.move(delta, **kw)


@pytest.mark.parametrize("key", C.SHIFT_KEYS)
@pytest.mark.parametrize("which", C.LISTS)
@pytest.mark.parametrize("form", C.DELTA_FORMS)
def test_carry(eng, twin, key, which, form):
    """duals and constants: bit for bit those of a twin that ran plain lpmp_move_windows; labels: ``model.move_labels``, unset
    entries unset, while the plain call on the twin still unsets — without costs, then (a second move) with them"""
    m = C.shift_model(key)
    lst = C.listed(m, which)
    bufs = _twins_after_passes(eng, twin, m)
    sets = [e.window_set(lst) for e in (eng, twin)]
    u = C.unaries(m)
    for step, with_costs in enumerate((False, True)):
        p = C.random_primal(m, 40 + step, unset_every=6)
        for e in (eng, twin):
            e.upload_primal(p)
        delta = C.deltas(m, lst, form, seed=step)
        sat = np.clip(delta, -C.MOVE_DELTA_MAX, C.MOVE_DELTA_MAX)
        costs = MW.cost_pair(m, C.rows(m, lst), sat, 50 + step, inf=True) if with_costs else None
        built = eng.schedules_built()
        keep = [_move(ws, delta, form, costs, carry) for ws, carry in zip(sets, (True, False))]
        assert eng.schedules_built() == built
        da, db = eng.download_duals(), twin.download_duals()
        assert not np.any(np.isnan(da)) and da.tobytes() == db.tobytes()
        ca, cb = bufs[0].cpu().numpy(), bufs[1].cpu().numpy()
        assert ca.tobytes() == cb.tobytes()
        got = eng.download_primal()
        want = M.move_labels(p, m, lst, delta)
        assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
        assert np.array_equal(got[u, 0] == m.f_dim0[u], p[u, 0] == m.f_dim0[u])
        assert np.array_equal(twin.download_primal(), C.unset_primal(m))      # the plain call still unsets
        assert _same(eng.lower_bound(), twin.lower_bound())
        del keep
    for ws in sets:
        ws.close()


@pytest.mark.parametrize("key", C.SHIFT_KEYS)
@pytest.mark.parametrize("which", C.LISTS)
@pytest.mark.parametrize("costs", (False, True))
def test_carry_keeps_the_primal_cost_where_nothing_clamps(eng, key, which, costs):
    m = C.shift_model(key)
    lst = C.listed(m, which)
    eng.upload(m)
    eng.set_reparametrization(ANISO)
    eng.compute_pass(2)
    ws = eng.window_set(lst)
    cell = Cell()
    for rep in range(3):
        p = C.random_primal(m, 60 + rep)
        eng.upload_primal(p)
        before = eng.evaluate_primal()
        assert np.isfinite(before)
        delta = C.no_clamp_deltas(m, lst, p, 70 + rep)
        assert np.any(delta != 0)
        if costs:
            # (any pair that agrees on the shared absolute labels keeps the energy: the term is skipped there and theta carried)
            co, cn = C.agreeing_costs(m, lst, delta, 80 + rep)
            ws.move(delta, cost_old=co, cost_new=cn, carry_labels=True)
        else:
            ws.move(delta, carry_labels=True)
        assert np.array_equal(eng.download_primal(), M.move_labels(p, m, lst, delta))
        after = eng.evaluate_primal()
        assert _same(before, after), (before, after)
        eng.evaluate_primal(cell.ptr)
        assert _same(cell.read(eng), before)
    ws.close()


def test_carry_without_a_primal_array_makes_none(eng):
    m = C.shift_model("shift24")
    eng.upload(m)
    eng.set_reparametrization(ANISO)
    eng.compute_pass(1)
    ws = eng.window_set()
    ws.move(C.deltas(m, None, "mixed"), carry_labels=True)
    r = eng.readout()
    u = C.unaries(m)
    assert np.array_equal(r.labels(), m.f_dim0[u])                            # all unset
    assert np.array_equal(eng.download_primal(), C.unset_primal(m))
    r.close(); ws.close()


def test_carry_refusals(eng):
    """the checks of lpmp_move_windows under the new name; a refused call writes nothing, the labels included"""
    m = C.shift_model("shift24")
    eng.upload(m)
    eng.set_reparametrization(ANISO)
    eng.compute_pass(1)
    p = C.random_primal(m, 90)
    eng.upload_primal(p)
    d = eng.download_duals()
    ws = eng.window_set()
    delta = C.deltas(m, None, "mixed")
    bad = delta.copy()
    bad[3] = C.MOVE_DELTA_MAX + 1
    _refused(C.INVALID, lambda: ws.move(bad, carry_labels=True), "lpmp_move_windows_carry", "entry 3")
    co, _ = C.agreeing_costs(m, None, delta, 1)
    _refused(C.INVALID, lambda: ws.move(delta, cost_old=co, carry_labels=True), "lpmp_move_windows_carry")
    assert np.array_equal(eng.download_primal(), p) and eng.download_duals().tobytes() == d.tobytes()
    eng.upload(m)
    _refused(C.STATE, lambda: ws.move(delta, carry_labels=True), "another model")
    ws.close()


# ---- the scalars -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", C.BOUND_SIZES)
def test_bound_of_isolated_factors(eng, twin, nf):
    """the isolated 2-label vector models of tests/test_bound_sum_gpu.py at every slice edge of the sum: the device bound equals the
    host bound by bits, on twin engines and on one engine (device call first, then host)"""
    m = BS.model(nf)
    cell = Cell()
    eng.upload(m)
    twin.upload(m)
    eng.lower_bound(cell.ptr)
    got = cell.read(eng)
    want = twin.lower_bound()
    assert np.isfinite(want) and _same(got, want), (got, want)
    assert _same(eng.lower_bound(), got)
    # once more, now on tracked bounds with a few stale entries across slice edges: the list kernel with its count on the device
    ch = BS._changed(nf)
    rows = BS.costs(len(ch), 7)
    for e in (eng, twin):
        e.set_vectors(ch, rows)
    recomputed = eng.lower_bound_recomputed()
    eng.lower_bound(cell.ptr)
    assert eng.lower_bound_recomputed() == recomputed                         # keeps the value of the last host call
    got = cell.read(eng)
    want = twin.lower_bound()
    assert _same(got, want) and _same(eng.lower_bound(), got), (got, want)


def _grid_pair(eng, twin, m, **kw):
    for e in (eng, twin):
        e.upload(m, **kw)
        e.set_reparametrization(ANISO)
        e.compute_pass(2)


def _bound_both(eng, twin, cell):
    """device call on one engine, host call on its twin, then the host call on the first: all three by bits"""
    eng.lower_bound(cell.ptr)
    got = cell.read(eng)
    want = twin.lower_bound()
    assert np.isfinite(want) and _same(got, want), (got, want)
    assert _same(eng.lower_bound(), want)
    return want


@pytest.mark.parametrize("layout", ("packed", "rows", "f32"))
def test_bound_on_a_grid_after_passes(eng, twin, layout):
    """nothing stale; one stale factor (the list path); more than an eighth stale (the host recomputes everything, the device call
    runs its list); all stale after upload_costs"""
    kw = {"rows": {"rows_layout": True}, "f32": {"table_precision": "f32_round"}, "packed": {}}[layout]
    m = S.grid_model(12, 10, 32 if layout != "rows" else 9, pairwise="dense", order="colour_major", seed=5)
    u = C.unaries(m)
    L = int(m.f_dim0[u[0]])
    cell = Cell()
    try:
        _grid_pair(eng, twin, m, **kw)
        _bound_both(eng, twin, cell)                                   # everything stale after the upload ... or tracked by the passes
        for e in (eng, twin):
            e.compute_pass(1)
        _bound_both(eng, twin, cell)                                           # nothing stale
        r = np.random.default_rng(3)
        one = r.random((1, L))
        for e in (eng, twin):
            e.set_vectors(u[17:18], one)
        _bound_both(eng, twin, cell)                                           # one stale factor
        assert twin.lower_bound_recomputed() == 1
        many = u[: m.n_factors // 8 + 3]
        rows = r.random((len(many), L))
        for e in (eng, twin):
            e.set_vectors(many, rows)
        _bound_both(eng, twin, cell)                                           # more than an eighth stale
        assert twin.lower_bound_recomputed() == m.n_factors and len(many) > m.n_factors // 8
        for e in (eng, twin):
            e.upload_costs(const=m.const_data)
        _bound_both(eng, twin, cell)                                           # all stale
        for e in (eng, twin):
            e.compute_pass(1)
        _bound_both(eng, twin, cell)
        assert np.array_equal(eng.download_duals(), twin.download_duals())
    finally:
        _defaults(eng, twin)


def test_bound_inside_a_batch_of_passes_that_ran_ahead(monkeypatch):
    """the solver loop compute_pass(1) + bound with passes running ahead: the device call answers from the row of the pass the
    caller is at and causes no rollback; the history equals that of an engine without speculation, by bits"""
    monkeypatch.setenv("LPMP_ROT_BANDS", "6")          # the joined chain on a small model (tests/test_speculation_gpu.py)
    m = S.grid_model(40, 36, 32, pairwise="dense", order="colour_major", seed=32)
    a, b = E.Engine(0), E.Engine(0)
    try:
        for e in (a, b):
            e.upload(m); e.set_reparametrization(ANISO)
            e.lower_bound()
        b.set_speculation(8)
        cells = [Cell() for _ in range(15)]
        hist_a = []
        for it in range(15):
            a.compute_pass(1); hist_a.append(a.lower_bound())
            b.compute_pass(1); b.lower_bound(cells[it].ptr)
        st = b.speculation_stats()
        assert st["batches"] == 4 and st["passes_used"] == 15 and st["passes_launched"] == 2 + 4 + 8 + 8 and st["rollbacks"] == 0, st
        hist_b = [c.read(b) for c in cells]            # (the first read settles: one pass of the last batch is unused)
        assert _bits(hist_a).tobytes() == _bits(hist_b).tobytes(), (hist_a, hist_b)
        assert np.array_equal(a.download_duals(), b.download_duals())
    finally:
        a.close(); b.close()


def test_primal_cost_on_the_device(eng, twin):
    """a consistent labelling; a stray pairwise slot through upload_primal and unset labels, both +inf; the status codes"""
    m = PM.grid(9, 7, 8, "colour_major")
    cell = Cell()
    fresh = E.Engine(0)
    try:
        _refused(C.STATE, lambda: fresh.evaluate_primal(cell.ptr))             # before an upload
        _refused(C.STATE, lambda: fresh.lower_bound(cell.ptr))
    finally:
        fresh.close()
    _grid_pair(eng, twin, m)
    assert eng.L.lpmp_evaluate_primal_dev(eng.h, None) == C.INVALID and eng.L.lpmp_lower_bound_dev(eng.h, None) == C.INVALID
    p = C.random_primal(m, 13)
    for e in (eng, twin):
        e.upload_primal(p)
    eng.evaluate_primal(cell.ptr)
    got, want = cell.read(eng), twin.evaluate_primal()
    assert np.isfinite(want) and _same(got, want) and _same(eng.evaluate_primal(), want), (got, want)
    stray = p.copy()
    pw = np.flatnonzero(m.f_kind != M.F_VECTOR)[5]
    stray[pw, 1] = (stray[pw, 1] + 1) % 8
    eng.upload_primal(stray)
    eng.evaluate_primal(cell.ptr)
    assert cell.read(eng) == np.inf and eng.evaluate_primal() == np.inf
    unset = C.random_primal(m, 13, unset_every=9)
    eng.upload_primal(unset)
    eng.evaluate_primal(cell.ptr)
    assert cell.read(eng) == np.inf and eng.evaluate_primal() == np.inf
    eng.upload_primal(p)                                                       # ... and back
    eng.evaluate_primal(cell.ptr)
    assert _same(cell.read(eng), want)
    assert cell.read(eng) >= twin.lower_bound() - 1e-9
