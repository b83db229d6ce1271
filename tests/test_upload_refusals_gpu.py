"""lpmp_upload_model builds the new model as a value and commits it at the end (csrc/engine.cpp; ModelState, csrc/engine_state.hpp): a refused upload leaves
NO model at whatever point it is refused, the engine's settings survive it, and nothing of an earlier model survives the next one.
Every case compares the engine that went through the refusal (or through a larger model) with a freshly created engine given the
same calls: duals, bound and labels bit for bit.  Model: a 4 x 4 grid with 3 labels and dense pairwise tables."""
import numpy as np
import pytest
import torch

from lp_mp_amd import engine as E, model as M, synthetic as S

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -2, -4
ANISO = M.REPAM_ANISOTROPIC


def grid(H=4, W=4, L=3, seed=1, flags=0, bad_entry=False, compute_primal=False, order="row_major"):
    """grid MRF whose costs are exactly floats (multiples of 1/64), so that every table precision takes it; ``bad_entry``: one
    table entry of 0.1, which f32-strict refuses; ``flags``: of both message types (M.MF_BATCH_TO_RIGHT: no residual sends)"""
    var = S.grid_variable_order(H, W, order).reshape(-1)
    a, bb = S.grid_edges(H, W)
    i, j = np.minimum(var[a], var[bb]), np.maximum(var[a], var[bb])
    mts = [M.MsgType(0, 1, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 0, flags), M.MsgType(0, 1, M.SCHED_LEFT, 0, 1, M.M_UNARY_PAIRWISE, 1, flags)]
    b = M.ModelBuilder(2, mts, [1, 0] if compute_primal else None)
    u = b.add_vector_factors(0, np.floor(S.u01(H * W * L, seed) * 64).reshape(-1, L) / 64)
    tables = np.floor(S.u01(len(a) * L * L, seed + 1) * 64).reshape(-1, L, L) / 64
    if bad_entry:
        tables[len(a) // 2, 1, 2] = 0.1
    p = b.add_dense_pairwise(1, tables)
    b.add_interleaved_messages(np.tile(np.array([0, 1], np.int32), len(a)), np.stack([u[i], u[j]], 1).reshape(-1), np.repeat(p, 2))
    b.add_relations(np.stack([u[i], p], 1).reshape(-1), np.stack([p, u[j]], 1).reshape(-1))
    return b.finish()


def refused(e, code, *args, **kw):
    """the upload fails with ``code``, and the engine holds no model afterwards"""
    with pytest.raises(E.EngineError) as ei:
        e.upload(*args, **kw)
    assert ei.value.code == code, ei.value
    with pytest.raises(E.EngineError) as ei:
        e.compute_pass(1)
    assert ei.value.code == ERR_STATE, ei.value


def three_passes(e):
    e.set_reparametrization(ANISO)
    e.compute_pass(3)
    return torch.from_numpy(e.download_duals()), e.lower_bound()


def same(got, want):
    assert torch.equal(got[0], want[0])
    assert got[1] == want[1], (got[1], want[1])


# every refusal point of lpmp_upload_model that the binding reaches.  A case sets what the upload needs, lets the upload be refused
# when ``refuse_first`` says so (the engine under test; the freshly created engine it is compared with skips that), then uploads the good model
def _f32_strict(e, refuse_first):
    if refuse_first:
        refused(e, ERR_UNSUPPORTED, grid(bad_entry=True), table_precision="f32")        # narrow_tables, tables from host memory
    e.upload(grid(), table_precision="f32")


def _f32_strict_device_tables(e, refuse_first):
    good, bad = grid(), grid(bad_entry=True)
    if refuse_first:
        t = torch.from_numpy(bad.const_data).cuda()
        refused(e, ERR_UNSUPPORTED, bad, const_dev=t.data_ptr(), keep=t, table_precision="f32")   # narrow_tables, the caller's device buffer
    t = torch.from_numpy(good.const_data).cuda()
    e.upload(good, const_dev=t.data_ptr(), keep=t, table_precision="f32")


def _f32_with_rows(e, refuse_first):
    if refuse_first:
        refused(e, ERR_UNSUPPORTED, grid(), table_precision="f32", rows_layout=True)
    e.upload(grid(), table_precision="f32", rows_layout=False)


def _send_rule(e, refuse_first):
    e.set_reparametrization_type(M.RTYPE_RESIDUAL)          # set beforehand: checked at the very end of the upload
    if refuse_first:
        refused(e, ERR_UNSUPPORTED, grid(flags=M.MF_BATCH_TO_RIGHT))
    e.upload(grid())


def _misaligned_device_tables(e, refuse_first):
    good = grid()
    if refuse_first:
        t = torch.zeros(good.const_data.shape[0] + 1, dtype=torch.float64, device="cuda")
        refused(e, ERR_INVALID, good, const_dev=t.data_ptr() + 8, keep=t)
    e.upload(good)


def _invalid_model(e, refuse_first):
    if refuse_first:
        import dataclasses
        good = grid()
        dims = good.f_dim0.copy(); dims[0] = 0                                   # the planner refuses it: a factor without labels
        refused(e, ERR_INVALID, dataclasses.replace(good, f_dim0=dims, _keep=[]))
    e.upload(grid())


@pytest.mark.parametrize("case", [_f32_strict, _f32_strict_device_tables, _f32_with_rows, _send_rule, _misaligned_device_tables, _invalid_model],
                         ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("held_a_model", [False, True], ids=["first_upload", "after_a_model"])
def test_a_refused_upload_leaves_no_model(case, held_a_model):
    e, f = E.Engine(0), E.Engine(0)
    try:
        if held_a_model:                # the refused upload has dropped this one: nothing of it answers afterwards either
            e.upload(grid(5, 4, 4, seed=7)); e.set_reparametrization(ANISO); e.compute_pass(1)
        case(e, refuse_first=True)
        case(f, refuse_first=False)
        same(three_passes(e), three_passes(f))
    finally:
        e.close(); f.close()


def test_settings_survive_a_refused_upload(monkeypatch):
    """set_speculation(4) and set_rows_layout(1) before a refused upload still hold for the next good one.  The rows layout keeps
    passes from running ahead (include/lpmp_engine.h), so the four single passes are counted twice: with the rows, where the engine
    must count what a fresh engine with the same settings counts, and after a second refused upload without them, where the header's
    rule says what four single passes are at depth 4: a batch of 2, then a batch of 4"""
    monkeypatch.setenv("LPMP_ROT_BANDS", "6")          # the joined chain on a small model (as tests/test_speculation_gpu.py does)
    m = grid(order="colour_major")
    e, f = E.Engine(0), E.Engine(0)
    try:
        for x in (e, f):
            x.set_speculation(4)
            assert x.L.lpmp_set_rows_layout(x.h, 1) == 0
        refused(e, ERR_UNSUPPORTED, grid(), table_precision="f32")      # f32 and the rows layout together
        for x in (e, f):
            x.upload(m, table_precision="f64")
            assert x.rows_layout
            x.set_reparametrization(ANISO)
            for k in range(4):
                x.compute_pass(1)
        assert e.speculation_stats() == f.speculation_stats() and e.speculation_stats()["batches"] == 0, e.speculation_stats()
        assert torch.equal(torch.from_numpy(e.download_duals()), torch.from_numpy(f.download_duals()))
        # ... and without the rows: the depth that was set before both refusals is still 4
        refused(e, ERR_UNSUPPORTED, grid(bad_entry=True), table_precision="f32", rows_layout=False)
        for x in (e, f):
            x.upload(m, table_precision="f64", rows_layout=False)
            assert not x.rows_layout
            x.set_reparametrization(ANISO)
            for k in range(4):
                x.compute_pass(1)
        st = e.speculation_stats()
        assert st == f.speculation_stats(), (st, f.speculation_stats())
        assert st["batches"] == 2 and st["passes_launched"] == 6 and st["passes_used"] == 4 and st["rollbacks"] == 0, st
        assert e.lower_bound() == f.lower_bound()
        assert torch.equal(torch.from_numpy(e.download_duals()), torch.from_numpy(f.download_duals()))
    finally:
        e.close(); f.close()


def test_nothing_of_a_larger_model_is_left(monkeypatch):
    """an engine that has held a 6 x 6 grid with 5 labels — in the rows layout with a primal pass, a decode and a read-out, then
    packed with an open batch of passes that ran ahead — gives on the small model what a fresh engine gives, and the read-out made
    for the old model answers LPMP_ERR_STATE"""
    monkeypatch.setenv("LPMP_ROT_BANDS", "6")
    big = grid(6, 6, 5, seed=3, compute_primal=True, order="colour_major")
    small = grid(compute_primal=True, order="colour_major")
    e, f = E.Engine(0), E.Engine(0)
    try:
        e.upload(big, rows_layout=True)
        assert e.rows_layout
        e.set_reparametrization(ANISO)
        e.compute_pass(2)
        e.compute_pass_and_primal(1)
        e.decode_primal(0, 1)
        r = e.readout()
        assert r.labels().shape == (36,) and r.beliefs().shape == (36, 5)
        e.upload(big, rows_layout=False)
        e.set_speculation(4)
        e.set_reparametrization(ANISO)
        e.compute_pass(1)
        opened = e.speculation_stats()["batches"]
        assert opened == 1, opened                        # the device is a pass ahead of the caller when the small model arrives
        f.set_speculation(4)
        got = []
        for x in (e, f):
            x.upload(small)
            duals, lb = three_passes(x)
            x.decode_primal(0, 1)
            got.append((duals, lb, x.download_primal(), x.readout().labels()))
        with pytest.raises(E.EngineError) as ei:
            r.labels()
        assert ei.value.code == ERR_STATE
        same(got[0][:2], got[1][:2])
        assert np.array_equal(got[0][2], got[1][2]) and np.array_equal(got[0][3], got[1][3])
        assert (got[0][3] < 3).all()                       # decoded: every unary has a label
    finally:
        e.close(); f.close()
