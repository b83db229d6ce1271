"""Every kernel family at constant and dual offsets past 2^31 elements (placement P31; the packed dense, packed Potts and streaming
dense families past 2^32 as well, P32).  tests/far_offset_cases.py puts tens of thousands of isolated, all-zero padding factors in
front of a small live model; the costs live in two borrowed device tensors of about 16 GiB (32 GiB) each, the live part at their
tails.  The far engine never moves its duals through the host: after ``synchronize()`` the tail of the borrowed dual tensor is
compared with the oracle's duals of the SMALL model, bit for bit, and both padding regions must still be all +0.0.

Besides the sweep families the module runs the calls large models make around them: shifted difference-indexed factors, joined
passes in every form (which one ran is read from the engine's counter), listed constants and the pool swap, prepared read-outs,
the decode (behind VECTOR padding: far duals, near constants — the only padding its planner accepts), moving label windows with
their write into the borrowed const buffer, and labeling lists whose left factor has several labelings.  What these calls compute
is compared with the numpy statements and the oracle of their own near tests, on the SMALL model.

Tolerances are those of tests/test_diff_tables_gpu.py.  The kernel class is asserted before anything runs.  Whether the planner
hands out the right offsets is tests/test_far_offsets_host.py; this module is about the kernels' index arithmetic."""
import dataclasses
import json
import re

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import far_offset_cases as F
import recost_cases as RC
from far_offset_gpu import (FLB_ATOL, LB_RTOL, SENTINEL_I32, Far, _buffers, _check_labels, _mem, _note, _release, _restart_oracle,  # noqa: F401
                            _sample_memory, _timed)

pytestmark = pytest.mark.gpu

ANISO, UNIFORM = M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM
MODES = (ANISO, UNIFORM)


@pytest.fixture(scope="module")
def p31():
    b = _buffers("P31")
    yield b
    _release(b)
    print("\nfar offsets: placements that ran: %s; peak device memory in use beyond the start of the module: %.1f GiB"
          % (sorted(_mem["ran"]), (_mem["free0"] - _mem["min_free"]) / F.GIB))
    print("far offsets: kernels per family: " + json.dumps(_mem["kernels"], sort_keys=True))


@pytest.fixture(scope="class")
def p32():
    b = _buffers("P32")
    yield b
    _release(b)


@pytest.fixture(scope="class")
def p31_vector():
    b = _buffers("P31", "vector")
    yield b
    _release(b)


@pytest.fixture(autouse=True)
def _memory_after_every_test():
    yield
    _sample_memory()


def _run(bufs, name, family, only=None, some=None, modes=MODES, kernel=None, **kw):
    m = F.live(name)
    for mode in modes:
        with Far(bufs, m, mode, **kw) as x:
            x.classes(only if only is not None else F.LIVE[name][1], some)
            kt = x.standard(family)
            if kernel is not None:
                assert any(v["kernel"].startswith(kernel) for v in kt.values()), (kernel, kt)
    return kt


# ---- the families of the table, placement P31 ---------------------------------------------------------------------------------
PACKED_DENSE = {"dense32": "sweep_dense_pk_kernel<32, 2, false", "dense8": "sweep_dense_pk_kernel<8, 4, false", "dense4": "sweep_dense_pk_kernel<4, 4, false",
                "dense_v21": "sweep_dense_pk_kernel<32, 2, true", "dense_v5": "sweep_dense_pk_kernel<8, 4, true"}
PACKED_POTTS = {"potts16": "sweep_potts_pk_kernel<16, false", "potts_v5": "sweep_potts_pk_kernel<8, true"}
STREAMING = {"big48": "sweep_dense_big_kernel", "big130": "sweep_dense_big_kernel"}


@pytest.mark.parametrize("nt", [0, 1], ids=["nt0", "nt1"])
@pytest.mark.parametrize("name", list(PACKED_DENSE))
def test_packed_dense_exact_and_var_both_access_policies(p31, name, nt, monkeypatch):
    monkeypatch.setenv("LPMP_NT", str(nt))
    kt = _run(p31, name, "packed dense", kernel=PACKED_DENSE[name])
    if name in ("dense32", "dense8", "dense4"):
        assert all(v["kernel"].endswith(", true>" if nt else ", false>") for v in kt.values()), kt


@pytest.mark.parametrize("name", list(PACKED_POTTS))
def test_packed_potts(p31, name):
    _run(p31, name, "packed potts", kernel=PACKED_POTTS[name])


@pytest.mark.parametrize("name", list(STREAMING))
def test_streaming_dense(p31, name):
    _run(p31, name, "streaming dense", kernel=STREAMING[name])


@pytest.mark.parametrize("name", ["shared32", "shared8"])
def test_shared_tables_in_lds(p31, name):
    assert F.live(name).n_shared_tables == 2
    _run(p31, name, "shared", kernel="sweep_shared_pk_kernel<%s" % name[6:])


def test_diff_full(p31):
    m = F.live("diff40")
    assert E.Plan(m).diff_band_info(0, ANISO)["band_launches"] == 0
    _run(p31, "diff40", "diff full", kernel="sweep_diff_kernel")


def test_diff_banded(p31):
    m = F.live("diff_band130")
    for mode in MODES:
        with Far(p31, m, mode) as x:
            x.classes({"diff"})
            assert x.e.plan.diff_band_info(0, mode)["band_launches"] > 0
            kt = x.standard("diff banded")
            assert kt["diff"]["band_launches"] > 0 and kt["diff"]["kernel"] == "sweep_diff_band_kernel", kt


@pytest.mark.parametrize("name", ["pairwise8_right", "pairwise8_full"])
def test_updated_pairwise_factors(p31, name):
    m = F.live(name)
    for mode in MODES:
        with Far(p31, m, mode) as x:
            for d in (0, 1):
                assert "pairwise8" in x.e.plan.schedule_classes(d, mode)
            kt = x.standard("updated pairwise")
            assert kt["pairwise8"]["kernel"] == "sweep_pairwise_pk_kernel<8>", kt


def test_generic_wave_per_factor_on_a_mixed_graph(p31):
    m = F.live("mixed_graph")
    assert {M.F_PAIRWISE_DENSE, M.F_PAIRWISE_POTTS, M.F_PAIRWISE_SHARED, M.F_PAIRWISE_DIFF} <= set(m.f_kind.tolist())
    kt = _run(p31, "mixed_graph", "generic wave", some={"generic"})
    assert kt["generic"]["kernel"] == "sweep_generic_kernel<64>", kt


def test_generic_lane_per_factor_on_a_labeling_list_model(p31):
    kt = _run(p31, "c5_small", "generic lane", some={"small"})
    assert kt["small"]["kernel"] == "sweep_generic_kernel<1>", kt


def test_generic_level_loop(p31, monkeypatch):
    """many tiny generic levels (a row-major grid whose DIFF factors are updated) as ONE launch of one workgroup that walks them;
    that the plan is a level loop: tests/test_far_offsets_host.py"""
    monkeypatch.delenv("LPMP_NO_CHAIN", raising=False); monkeypatch.delenv("LPMP_NO_LEVEL_LOOP", raising=False)
    m = F.live("level_loop40")
    for mode in MODES:
        with Far(p31, m, mode) as x:
            x.classes(some={"generic"})
            for d in (M.FORWARD, M.BACKWARD, -1):
                assert x.e.plan.chain_info(d, mode)["n_chains"] == 1
            x.bound("upload")
            for k in range(3):
                x.e.compute_pass(1); x.o.ComputePass(1)      # (not timed: per-launch timing runs the levels launch by launch)
                x.bound(k)
            x.e.forward_pass(); x.o.ComputeForwardPass()
            x.e.backward_pass(); x.o.ComputeBackwardPass()
            x.e.compute_pass(2); x.o.ComputePass(2)
            x.duals()
            x.factor_bounds()
            x.padding_untouched()
    _mem["kernels"].setdefault("level loop", ["level_loop_kernel<64> (the chain form of class generic; not timed)"])


# ---- chain executor ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["joined_dense32", "joined_potts8"])
def test_joined_passes_as_one_blocked_chain_launch(p31, name, monkeypatch):
    """the engine's default form: peer minima for the dense grid (every chain launch, by the counter), the blocked chain of the packed
    Potts class, which has no other form, for the Potts grid.  The forms behind the switches: test_joined_passes_in_every_form"""
    _pq_env(monkeypatch, {})
    monkeypatch.setenv("LPMP_ROT_BANDS", "8"); monkeypatch.setenv("LPMP_ROT_LAG", "2"); monkeypatch.setenv("LPMP_ROT_DEPTH", "4")
    with Far(p31, F.live(name), ANISO) as x:
        x.classes(F.LIVE[name][1])
        assert x.e.plan.pass_rotates(ANISO)
        assert x.e.plan.peer_minima(ANISO)[0] == (name == "joined_dense32")
        for n in (1, 5, 2):
            kt = x.timed_passes(n, "joined passes")
            assert all(v["kernel"].startswith("chain_") and v["chain_launches"] == 1 for v in kt.values()), kt
            assert x.e.peer_minima_launches() == (1 if name == "joined_dense32" else 0), (n, kt)
            x.duals(n)
            x.bound(n)
        x.factor_bounds()
        x.padding_untouched()


@pytest.mark.parametrize("mailbox", [True, False], ids=["mailbox", "flags"])
@pytest.mark.parametrize("name", ["deep_dense16", "deep_potts8"])
def test_deep_chains_with_and_without_the_mailbox(p31, name, mailbox, monkeypatch):
    monkeypatch.delenv("LPMP_NO_CHAIN", raising=False)
    if mailbox:
        monkeypatch.delenv("LPMP_NO_MAILBOX", raising=False)
    else:
        monkeypatch.setenv("LPMP_NO_MAILBOX", "1")
    for mode in MODES:
        with Far(p31, F.live(name), mode) as x:
            x.classes(F.LIVE[name][1])
            ci = x.e.plan.chain_info(M.FORWARD, mode)
            assert ci["n_chains"] == 1 and (ci["mailbox_rows"] > 0) == mailbox, ci
            for n in (1, 3):
                x.e.compute_pass(n); x.o.ComputePass(n)
                x.bound(n)
            x.e.forward_pass(); x.o.ComputeForwardPass()
            x.e.backward_pass(); x.o.ComputeBackwardPass()
            x.duals()
            x.factor_bounds()
            x.padding_untouched()
    _mem["kernels"].setdefault("deep chains", ["chain form of class %s (not timed: timing runs launch by launch)" % sorted(F.LIVE[name][1])[0]])


# ---- float tables narrowed out of the borrowed buffer -----------------------------------------------------------------------
@pytest.mark.parametrize("name,kernel", [("dense32", "sweep_dense_pk_f32_kernel<32, 2, false"), ("big48", "sweep_dense_big_f32_kernel")])
def test_float_tables_from_the_borrowed_buffer(p31, name, kernel):
    m = F.live(name)
    assert np.any(m.const_data.astype(np.float32).astype(np.float64) != m.const_data)
    for mode in MODES:
        with Far(p31, m, mode, oracle_of=lambda s: s.with_f32_tables(), table_precision="f32_round") as x:
            assert x.e.table_precision() == "f32_round"
            x.classes(F.LIVE[name][1])
            kt = x.standard("float tables")
            assert any(v["kernel"].startswith(kernel) for v in kt.values()), kt


# ---- behind vector padding (far duals, near constants): the rows layout and the decode -----------------------------------------
class TestRowsLayout:
    def test_rows_layout_behind_vector_padding(self, p31_vector):
        m = F.live("dense8")
        for mode in MODES:
            with Far(p31_vector, m, mode, rows_layout=True) as x:
                assert x.e.rows_layout
                x.classes({"dense8"})
                x.standard("rows layout")       # duals(): after synchronize() the packed tail holds the oracle's duals

    @pytest.mark.parametrize("name", ["dense8", "dense_v21", "big130", "shared32", "diff_shift40"])
    def test_decode_behind_vector_padding(self, p31_vector, name):
        """Far duals, near constants: the decode planner refuses isolated pairwise factors ("a side that has no unary"), so vector
        padding is the only padding a far decode can run behind (tests/test_far_offsets_host.py pins both).  Every padding unary
        is decoded, too: 65 536 all-zero labels, walked chunk by chunk by the wave-per-unary kernel, first minimiser 0"""
        import decode_cases as DC
        import readout_cases as R
        m = F.live(name)
        us = np.asarray(R.unaries(m), np.int32)
        small = E.Plan(m)
        with Far(p31_vector, m, ANISO) as x:
            e, n_pad = x.e, x.n_pad
            x.classes(F.LIVE[name][1])
            info = e.plan.decode_info(0)
            assert info["n_unaries"] == len(us) + n_pad and info["n_levels"] == small.decode_info(0)["n_levels"]
            e.compute_pass(2); x.o.ComputePass(2)
            d = x.duals()
            r = e.readout(us + n_pad)
            for direction in (0, 1):
                order = small.order(direction)
                for refine in (0, 1):
                    what = (name, direction, refine)
                    e.decode_primal(direction, refine)
                    got = e.download_primal()
                    want = DC.decode_reference(m, d, order, refine)
                    assert np.array_equal(got[n_pad:], want), (what, np.argwhere(got[n_pad:] != want)[:8].tolist())
                    assert not got[:n_pad].any(), what                          # every padding unary: label 0
                    assert e.check_primal_consistency()
                    cost, energy = e.evaluate_primal(), DC.energy(m, want)
                    assert abs(cost - energy) <= 1e-9 * max(1.0, abs(energy)), (what, cost, energy)
                    assert np.array_equal(r.labels(), want[us, 0]), what
                    e.synchronize()
                    assert np.array_equal(p31_vector.dual_tail(), d), what      # the decode reads only
            r.close()
            x.padding_untouched()
        L = int(m.f_dim0[us].max())
        _note("decode", "decode_kernel<64, 4> (the padding unaries)", "decode_kernel<%s> (%d labels)" % ("64, 4" if L > 64 else "64, 1" if L > 32 else "%d, 1" % max(4, 1 << (L - 1).bit_length()), L))


def send_only_updates(o, mode):
    """(factors, om_off, om, mk_off, mk): the updates of the oracle's forward sweep under ``mode`` with no active receive and at
    least one active send, in sweep order, each with its own weight and mask rows"""
    upd = o.update_order(M.FORWARD)
    oo, om = o.omega(M.FORWARD, mode)
    mo, mk = o.mask(M.FORWARD, mode)
    keep = [i for i in range(len(upd)) if not mk[mo[i]:mo[i + 1]].any() and (om[oo[i]:oo[i + 1]] != 0.0).any()]
    cat = lambda a, off, dt: np.concatenate([a[off[i]:off[i + 1]] for i in keep]).astype(dt) if keep else np.zeros(0, dt)
    offs = lambda off: np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in keep])]).astype(np.int64)
    return np.asarray(upd[keep], np.int32), offs(oo), cat(om, oo, np.float64), offs(mo), cat(mk, mo, np.uint8)


# ---- bounds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense8", "halo16", "dense32", "big48", "potts16", "shared32", "diff40", "mixed_graph"])
def test_full_and_list_bound_kernels(p31, name):
    m = F.live(name)
    with Far(p31, m, ANISO) as x:
        nf = x.far.n_factors
        x.e.compute_pass(1); x.o.ComputePass(1)
        x.e.invalidate_lower_bounds()
        x.factor_bounds("full")                          # dense_lb_kernel<8 / 16 / 32> on the square live factors, factor_lb_kernel on the rest
        assert x.e.lower_bound_recomputed() == nf
        x.bound("full")
        # a pass that keeps tracked bounds and leaves some stale: the updates of the forward sweep that receive nothing and send, with
        # their rows of that sweep, as an iterator-range pass.  A send that follows no receive of its own record marks the bound of
        # its peer NaN in every kernel class (after a whole pass, or a whole sweep, the packed classes have tracked every bound and
        # nothing is left for the list kernel)
        rows = send_only_updates(x.o, ANISO)      # (the first colour of a grid: under uniform weights every update receives)
        assert len(rows[0]) > 0
        x.e.compute_pass_custom(rows[0] + x.n_pad, *rows[1:]); x.o.compute_pass_custom(*rows)
        x.factor_bounds("list")
        n = x.e.lower_bound_recomputed()
        print(name, "bounds recomputed by the list kernel:", n, "of", nf)
        assert 0 < n <= nf // 8
        x.bound("list")
        x.duals()
        x.padding_untouched()


# ---- primal -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["primal_dense8", "primal_potts8"])
def test_primal_rounding(p31, name):
    m = F.live(name)
    for mode in MODES:
        with Far(p31, m, mode) as x:
            x.classes(F.LIVE[name][1])
            for it in range(3):
                x.e.compute_pass_and_primal(it); x.o.ComputePassAndPrimal(it)
                p = x.e.download_primal()
                assert np.array_equal(p[x.n_pad:], x.o.primal()), (mode, it)
                assert x.e.check_primal_consistency() == x.o.CheckPrimalConsistency()
                # no pass labels an isolated factor: the padding is labelled here, (0, 0) at cost 0.0 each — unset it would make the sum +inf
                assert np.all(p[:x.n_pad, 0] == 1) and np.all(p[:x.n_pad, 1] == F.PAD_LABELS)
                p[:x.n_pad] = 0
                x.e.upload_primal(p)
                c, co = x.e.evaluate_primal(), x.o.EvaluatePrimal()
                assert (c == co) if np.isinf(co) else abs(c - co) <= 1e-9 * max(1.0, abs(co)), (c, co)
                p[:x.n_pad] = (1, F.PAD_LABELS)
                x.e.upload_primal(p)
                x.duals((mode, it))
                x.e.compute_pass(1); x.o.ComputePass(1)
            x.padding_untouched()


# ---- new costs --------------------------------------------------------------------------------------------------------------
def test_new_costs_on_the_far_plan(p31):
    A = F.live("recost13")
    B = RC.recost(A, 1013)
    vec = np.flatnonzero(A.f_kind == M.F_VECTOR)
    with Far(p31, A, ANISO) as x:
        e, n_pad = x.e, x.n_pad
        for _ in range(2):                         # single passes: the schedule the passes after the new costs run is built here
            e.compute_pass(1); x.o.ComputePass(1)
        e.lower_bound()
        before = x.duals("passes on A")
        built, handle = e.schedules_built(), e.plan.h
        assert built > 0
        # set_vectors, plain and accumulate, some factors and not in factor order
        e.invalidate_lower_bounds(); e.lower_bound()      # from here on no bound is one a sweep kernel tracked (tests/test_recost_gpu.py, _prime)
        some = vec[[3, 17, 0, 41, 20]]
        rows = S.u01(len(some) * 16, 82).reshape(len(some), 16)                  # stride 16 > 13 labels
        for accumulate in (False, True):
            e.set_vectors(some + n_pad, rows, accumulate=accumulate)
            want = RC.scatter_rows(A, before, some, rows, accumulate)
            e.synchronize()
            assert np.array_equal(p31.dual_tail(), want), accumulate
            lb = e.lower_bound()
            assert 0 < e.lower_bound_recomputed() <= len(some)
            e.invalidate_lower_bounds()
            assert e.lower_bound() == lb
            before = want
        # zero_pairwise_duals
        e.zero_pairwise_duals()
        want = RC.zero_pairwise(A, before)
        e.synchronize()
        got = p31.dual_tail()
        assert np.array_equal(got, want) and not np.any(np.signbit(got[~RC.vector_mask(A)]))
        assert p31.dual_padding_nonzero() == 0
        # upload_costs of the same pointer after the tail was rewritten in place: a warm start on B's constants
        p31.write_const(B.const_data)
        e.upload_costs(const_dev=p31.const.data_ptr())
        assert e.plan.h == handle and e.schedules_built() == built
        start = dataclasses.replace(B, dual_data=want, _keep=[])
        x.o = Oracle(start); x.o.set_reparametrization(ANISO)
        x.m = start
        x.bound("warm start")
        for k in range(2):
            e.compute_pass(1); x.o.ComputePass(1)
            x.bound(k)
        x.duals("after the new costs")
        x.factor_bounds()
        assert e.schedules_built() == built
        x.padding_untouched()


# ---- boundary and halo kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["halo16", "halo40"])
def test_halo_and_boundary_kernels(p31, name):
    """halo_copy_kernel<16> (vectors of at most 16 doubles) and <64>; the boundary step against the numpy statement of the comment at
    the top of csrc/boundary.hip, the replies with the same order of additions"""
    import torch
    m = F.live(name)
    L = int(m.f_dim0[0])
    off = m.dual_offsets()
    pw = np.flatnonzero(m.f_kind != M.F_VECTOR)
    vec = np.flatnonzero(m.f_kind == M.F_VECTOR)
    rng = np.random.default_rng(L)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    with Far(p31, m, ANISO) as x:
        e, pad_d = x.e, p31.pad_d
        e.compute_pass(1); x.o.ComputePass(1)
        d = x.duals("one pass")
        # the live pairwise message vectors: side 0 of some factors, side 1 of others
        out = np.array([off[p] + (L if k % 2 else 0) for k, p in enumerate(pw[::2])], np.int64)
        inn = np.array([off[p] + (0 if k % 2 else L) for k, p in enumerate(pw[1::2])], np.int64)
        ln = lambda a: np.full(len(a), L, np.int32)
        assert np.any(d[(out[:, None] + np.arange(L)).reshape(-1)] != 0.0)
        h = e.halo_create(out + pad_d, ln(out), inn + pad_d, ln(inn))
        assert e.halo_sizes(h) == (len(out) * L, len(inn) * L)
        buf = torch.zeros(len(out) * L, dtype=torch.float64, device="cuda")
        e.halo_pack(h, buf.data_ptr()); e.synchronize(); torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), d[(out[:, None] + np.arange(L)).reshape(-1)])
        assert np.array_equal(p31.dual_tail(), d)
        data = rng.uniform(-1, 1, len(inn) * L)
        t = dev(data); torch.cuda.synchronize()
        e.halo_unpack(h, t.data_ptr()); e.synchronize()
        d[(inn[:, None] + np.arange(L)).reshape(-1)] = data
        assert np.array_equal(p31.dual_tail(), d)
        e.halo_destroy(h)
        # boundary: ghosts = the outgoing vectors above; 2 - 3 incoming messages per boundary variable, exchange order shuffled
        var = vec[:8]
        msg_var = np.repeat(np.arange(len(var)), [2 + k % 2 for k in range(len(var))])
        msg_var = msg_var[rng.permutation(len(msg_var))]                     # exchange order
        n_in = len(msg_var)
        omega = rng.uniform(0.1, 0.4, n_in)
        in_order = np.concatenate([np.flatnonzero(msg_var == v) for v in range(len(var))]).astype(np.int64)
        b = e.boundary_create(out + pad_d, ln(out), off[var[msg_var]] + pad_d, np.full(n_in, L, np.int32), omega, in_order)
        assert e.boundary_sizes(b) == (len(out) * L, n_in * L)
        send = torch.zeros(len(out) * L, dtype=torch.float64, device="cuda")
        e.boundary_pack(b, send.data_ptr()); e.synchronize(); torch.cuda.synchronize()
        idx = (out[:, None] + np.arange(L)).reshape(-1)
        assert np.array_equal(send.cpu().numpy(), d[idx])
        d[idx] = 0.0
        got = p31.dual_tail()
        assert np.array_equal(got, d) and not np.any(np.signbit(got[idx]))    # packed ghosts zeroed
        recv = rng.uniform(-1, 1, n_in * L)
        r, reply = dev(recv), torch.zeros(n_in * L, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        e.boundary_reply(b, r.data_ptr(), reply.data_ptr()); e.synchronize(); torch.cuda.synchronize()
        want_reply = np.zeros(n_in * L)
        for v in range(len(var)):
            th = d[off[var[v]]: off[var[v]] + L].copy()
            ms = np.flatnonzero(msg_var == v)
            for k in ms:
                th = th + recv[k * L: (k + 1) * L]
            snap = th.copy()
            for k in ms:
                rk = omega[k] * snap
                want_reply[k * L: (k + 1) * L] = rk
                th = th - rk
            d[off[var[v]]: off[var[v]] + L] = th
        assert np.array_equal(reply.cpu().numpy(), want_reply)
        assert np.array_equal(p31.dual_tail(), d)
        back = rng.uniform(-1, 1, len(out) * L)
        t = dev(back); torch.cuda.synchronize()
        e.boundary_fold(b, t.data_ptr()); e.synchronize()
        d[idx] = back
        assert np.array_equal(p31.dual_tail(), d)
        e.boundary_destroy(b)
        x.padding_untouched()
    _mem["kernels"].setdefault("boundary / halo", ["halo_copy_kernel<16> (16 labels) and <64> (40 labels), boundary_pack / reply / fold kernels (not timed by kernel_timing)"])


# ---- the kernels that came after the first far-offset tests -----------------------------------------------------------------
# Each family is a function over the buffers of a placement: the P31 tests below and the methods of TestP32 call the same one.
UNSUPPORTED = -2
SENTINEL = np.array([0x7FF8DEAD0000BEEF], np.uint64).view(np.float64)[0]      # a NaN with a payload (tests/test_readout_gpu.py)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- shifted difference-indexed factors -------------------------------------------------------------------------------------
def _diff_shift_sweep(bufs, name, family):
    m = F.live(name)
    only = F.LIVE[name][1]
    for mode in MODES:
        with Far(bufs, m, mode) as x:
            x.classes(only, None if only else {"generic"})
            kt = _timed(x, lambda: (x.e.forward_pass(), x.o.ComputeForwardPass()), family)
            if only:
                assert set(kt) == {"diff"} and kt["diff"]["kernel"] == "sweep_diff_shift_kernel", kt
                assert kt["diff"]["band_launches"] == 0 and kt["diff"]["shift_launches"] == kt["diff"]["launches"] > 0, kt
            else:      # DIFF_SHIFT beside DIFF, SHARED, DENSE and POTTS peers of one record: the wave-per-factor kernel reads all of them
                assert kt["generic"]["kernel"] == "sweep_generic_kernel<64>", kt
            x.duals("forward")
            kt = x.standard(family)
            if only:
                assert kt["diff"]["kernel"] == "sweep_diff_shift_kernel" and kt["diff"]["shift_launches"] > 0, kt


@pytest.mark.parametrize("name", F.DIFF_SHIFT_MODELS)
def test_diff_shift_sweep(p31, name):
    if name == "diff_shift_mixed":
        assert M.F_PAIRWISE_DIFF_SHIFT in set(F.live(name).f_kind.tolist())
    _diff_shift_sweep(p31, name, "diff shift")


# ---- joined passes in every form --------------------------------------------------------------------------------------------
PQ_KEYS = ("LPMP_PQ_WIDE", "LPMP_PQ_LDS", "LPMP_PQ_HOLD", "LPMP_PQ_SCATTER", "LPMP_NO_PEER_MINIMA", "LPMP_PQ_AHEAD", "LPMP_PQ_DESC_INLINE")
# name -> (environment of the engine, whether its joined passes run in the peer-minima form)
PQ_ENGINES = {"default": ({}, True), "wide0": ({"LPMP_PQ_WIDE": "0"}, True), "lds0": ({"LPMP_PQ_LDS": "0"}, True), "hold2": ({"LPMP_PQ_HOLD": "2"}, True),
              "scatter0": ({"LPMP_PQ_SCATTER": "0"}, True), "no_peer_minima": ({"LPMP_NO_PEER_MINIMA": "1"}, False),
              "ahead0": ({"LPMP_PQ_AHEAD": "0"}, True), "inline0": ({"LPMP_PQ_DESC_INLINE": "0"}, True)}
# the ticket form the verbose line of a peer-minima launch must name: tickets ahead (chain_dense_pq_ahead_kernel) is the default form
# and has no other switch turned; every other peer-minima form keeps the plain loop (kernels.hpp, pq_ahead_applies)
PQ_TICKETS = {"default": "ahead", "inline0": "ahead", "ahead0": "plain", "wide0": "plain", "hold2": "plain", "lds0": "plain", "scatter0": "plain"}
PQ_TICKET_LINE = re.compile(r"lpmp:   peer minima launch; tickets: (ahead|plain)")
PQ_LAUNCH_LINE = re.compile(r"lpmp: \d+ passes as one launch( \([a-z ,]+\))?: \d+ tickets")
PQ_PASSES = (1, 2, 9, 33)                    # explicit lists, the periodic template, a slice of 32 + 1
JOINED_WINDOW = (8, 2, 4)                    # bands : lag : depth, as tests/test_peer_minima_shapes_gpu.py runs both models
JOINED_KERNEL = "chain_dense_pk_kernel<32, 2, false, false>"          # the class's name in the timing, whichever form ran
# the skewed tiled order at test size (tests/test_pq_ahead_gpu.py SKEW, on its 24 x 24 grid of 32 labels)
SKEW = {"LPMP_ROT_BANDS": "8", "LPMP_ROT_LAG": "2", "LPMP_PQ_TILES": "4", "LPMP_PQ_SUB": "3", "LPMP_PQ_SUBLAG": "2", "LPMP_PQ_SUBGAP": "2"}
SKEW_KEYS = ("LPMP_ROT_BANDS", "LPMP_ROT_LAG", "LPMP_ROT_DEPTH", "LPMP_ROT_TILES", "LPMP_PQ_TILES", "LPMP_PQ_SUB", "LPMP_PQ_SUBLAG", "LPMP_PQ_SUBGAP",
             "LPMP_PQ_MIN_PASSES", "LPMP_CHAIN_MAX_WGS")
SKEW_CALLS = (20, 8)
SKEW_MIN_PASSES = 12                         # the shipped threshold (tests/test_pq_tiles_gpu.py)
_TRAJECTORY = {}


def _pq_env(monkeypatch, env):
    """the switches are read when an engine is created"""
    for k in PQ_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _joined_trajectory(name, calls=PQ_PASSES):
    """the oracle on the small model over ``calls``, computed once and left unchanged: (duals, bound) after every call, the factors'
    bounds at the end (the form of a launch changes nothing in what it computes)"""
    if (name, calls) not in _TRAJECTORY:
        m = F.live(name)
        o = Oracle(m); o.set_reparametrization(ANISO)
        steps = []
        for n in calls:
            o.ComputePass(n)
            d = o.duals().copy(); d.setflags(write=False)
            steps.append((d, o.LowerBound()))
        flb = np.array([o.factor_lower_bound(f) for f in range(m.n_factors)]); flb.setflags(write=False)
        _TRAJECTORY[(name, calls)] = (steps, flb)
    return _TRAJECTORY[(name, calls)]


def _joined_calls(x, bufs, engine, pq, calls, steps, flb, capfd, order=None):
    """the calls on one far engine against the trajectory; returns the duals after every call.  The verbose lines of the launches
    built on the way name the ticket form (and the order, where ``order`` is asked for): a fallback cannot stand in"""
    forms, orders, out = [], [], []
    for n, (duals, bound) in zip(calls, steps):
        capfd.readouterr()
        kt = _timed(x, lambda: x.e.compute_pass(n), "joined passes, " + engine)
        err = capfd.readouterr().err
        forms += PQ_TICKET_LINE.findall(err)
        orders.append((n, PQ_LAUNCH_LINE.findall(err)))
        (v,) = kt.values()
        assert v["kernel"] == JOINED_KERNEL and v["chain_launches"] == (n + 31) // 32, (engine, n, kt)
        assert v["peer_minima_launches"] == (v["chain_launches"] if pq else 0), (engine, n, kt)
        _note("joined passes, " + engine, "peer-minima launches: %s" % ("all" if pq else "none"))
        x.e.synchronize()
        d = bufs.dual_tail()
        assert np.array_equal(d, duals), (engine, n, float(np.max(np.abs(d - duals))))
        lb = x.e.lower_bound()
        assert np.isfinite(lb) and abs(lb - bound) <= LB_RTOL * max(1.0, abs(bound)), (engine, n, lb, bound)
        out.append((d, lb))
    got = x.e.factor_lower_bounds()
    assert np.all(got[:x.n_pad] == 0.0) and np.max(np.abs(got[x.n_pad:] - flb)) <= FLB_ATOL, engine
    x.padding_untouched()
    want = PQ_TICKETS.get(engine)
    print("joined passes, %s: ticket forms of the launches built: %s%s" % (engine, forms, orders if order else ""))
    if pq:
        assert forms and set(forms) == {want}, (engine, forms, want)
        _note("joined passes, " + engine, "tickets: %s (%s)" % (want, "chain_dense_pq_ahead_kernel" if want == "ahead" else "the plain ticket loop"))
    else:
        assert not forms, (engine, forms)
    if order:      # calls of at least SKEW_MIN_PASSES passes take the order; a shorter call builds its template in the band order
        long = [o for n, built in orders if n >= SKEW_MIN_PASSES for o in built]
        assert long and all(order in o and "periodic template" in o for o in long), (engine, orders)
        _note("joined passes, " + engine, "periodic template, " + order)
    return out


def _joined_passes(bufs, name, engine, monkeypatch, capfd):
    env, pq = PQ_ENGINES[engine]
    _pq_env(monkeypatch, env)
    for k, v in zip(("LPMP_ROT_BANDS", "LPMP_ROT_LAG", "LPMP_ROT_DEPTH"), JOINED_WINDOW):
        monkeypatch.setenv(k, str(v))
    monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
    steps, flb = _joined_trajectory(name)
    with Far(bufs, F.live(name), ANISO, oracle_of=None) as x:
        x.classes({"dense32"})
        assert x.e.plan.pass_rotates(ANISO) and x.e.plan.peer_minima(ANISO) == (True, "")
        _joined_calls(x, bufs, engine, pq, PQ_PASSES, steps, flb, capfd)


@pytest.mark.parametrize("engine", list(PQ_ENGINES))
@pytest.mark.parametrize("name", ["joined_dense32", "pq_mixed_sides"])
def test_joined_passes_in_every_form(p31, name, engine, monkeypatch, capfd):
    """peer minima as it is by default (tickets ahead), with each of its switches turned — the plain ticket loop, every dependency
    through dep[] — and the joined form it replaced (what float tables, the rows layout and LPMP_NO_PEER_MINIMA run): which form ran
    is read from the engine's counter, which tickets from the verbose line of every launch built"""
    _joined_passes(p31, name, engine, monkeypatch, capfd)


def test_joined_passes_in_the_skewed_tiled_order(p31, monkeypatch, capfd):
    """the skewed tiled order with its periodic template and flag ring, tickets ahead and LPMP_PQ_AHEAD=0 side by side on calls of 20
    and 8 passes: duals bit-equal to the oracle's trajectory and between the two engines, bounds as in every joined test"""
    name = "skew_dense32"
    steps, flb = _joined_trajectory(name, SKEW_CALLS)
    got = {}
    for engine in ("default", "ahead0"):
        env, pq = PQ_ENGINES[engine]
        _pq_env(monkeypatch, env)
        for k in SKEW_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in SKEW.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("LPMP_ROT_VERBOSE", "1")
        with Far(p31, F.live(name), ANISO, oracle_of=None) as x:
            x.classes({"dense32"})
            assert x.e.plan.pass_rotates(ANISO) and x.e.plan.peer_minima(ANISO) == (True, "")
            got[engine] = _joined_calls(x, p31, engine, pq, SKEW_CALLS, steps, flb, capfd, order="skewed tiled order")
    for (da, la), (db, lb) in zip(got["default"], got["ahead0"]):
        assert np.array_equal(da, db) and la == lb, (la, lb)


# ---- listed constants and the pool ------------------------------------------------------------------------------------------
def test_set_constants_from_host_and_device_rows(p31):
    import torch
    import repool_cases as RP
    m = F.live("diff_shift_mixed")
    fs = RP.listed_subset_shift(m, 3, share=2)
    assert {M.F_PAIRWISE_DIFF_SHIFT, M.F_PAIRWISE_DIFF, M.F_PAIRWISE_SHARED, M.F_PAIRWISE_DENSE, M.F_PAIRWISE_POTTS} == set(m.f_kind[fs].tolist())
    rows = RP.rows_for_shift(m, fs, 21)
    stride = rows.shape[1] + 5                                      # a device source with a stride above the longest row
    rows_dev = RP.rows_for_shift(m, fs, 22, stride=stride)
    with Far(p31, m, ANISO) as x:
        e = x.e
        for n in (1, 2):                                            # the schedules of both calls are built here
            e.compute_pass(n); x.o.ComputePass(n)
        d = x.duals("passes on the first constants")
        built, handle = e.schedules_built(), e.plan.h
        for source, r in (("host", rows), ("device", rows_dev)):
            if source == "device":
                t = torch.from_numpy(np.ascontiguousarray(r)).cuda(); torch.cuda.synchronize()
                e.set_constants(fs + x.n_pad, src_dev=t.data_ptr(), src_stride=stride)
            else:
                e.set_constants(fs + x.n_pad, r)
            new = RP.with_rows(x.m, fs, r)
            assert not np.array_equal(new.const_data, x.m.const_data)
            e.synchronize()
            assert np.array_equal(p31.const_tail(), new.const_data), source        # the borrowed buffer holds the new rows
            assert np.array_equal(p31.dual_tail(), d), source
            _restart_oracle(x, new, d)
            x.bound(source)
            e.compute_pass(2); x.o.ComputePass(2)
            d = x.duals(source)
            x.bound(source)
            x.factor_bounds(source)
            assert e.plan.h == handle and e.schedules_built() == built, source
        x.padding_untouched(const_tail=False)
        assert np.array_equal(p31.const_tail(), x.m.const_data)
    _note("set_constants", "set_constants_kernel (cells and packed scalars of SHARED / DIFF / DIFF_SHIFT factors, dense tables, Potts scalars)")


def test_set_constants_on_float_tables(p31):
    """f32_round: the rows are narrowed into the float tables (the check kernel runs first), the borrowed doubles stay; strict f32: a
    row that is not float-valued is refused and nothing is written"""
    import repool_cases as RP
    m = F.live("recost13")
    fs = RP.listed_subset(m, 5)
    rows = RP.rows_for(m, fs, 31)
    assert np.any(rows.astype(np.float32).astype(np.float64) != rows)
    with Far(p31, m, ANISO, oracle_of=lambda s: s.with_f32_tables(), table_precision="f32_round") as x:
        e = x.e
        assert e.table_precision() == "f32_round"
        x.classes(F.LIVE["recost13"][1])
        e.compute_pass(2); x.o.ComputePass(2)
        d = x.duals()
        built = e.schedules_built()
        e.set_constants(fs + x.n_pad, rows)
        _restart_oracle(x, RP.with_rows(m, fs, rows).with_f32_tables(), d)
        x.bound("rounded rows")
        e.compute_pass(2); x.o.ComputePass(2)
        x.duals("rounded rows"); x.bound("after two passes"); x.factor_bounds()
        assert e.schedules_built() == built
        x.m = m
        x.padding_untouched()                                       # the doubles of the borrowed buffer are never written
    A = m.with_f32_tables()
    with Far(p31, A, ANISO, table_precision="f32") as x:
        e = x.e
        assert e.table_precision() == "f32"
        e.compute_pass(2); x.o.ComputePass(2)
        d = x.duals()
        with pytest.raises(E.EngineError) as ei:
            e.set_constants(fs + x.n_pad, rows)
        assert ei.value.code == UNSUPPORTED and "nothing was written" in str(ei.value), str(ei.value)
        e.compute_pass(1); x.o.ComputePass(1)
        x.duals("after the refusal"); x.bound("after the refusal")
        exact = RP.rows_for(m, fs, 31, float_valued=True)
        d = x.duals()
        e.set_constants(fs + x.n_pad, exact)
        _restart_oracle(x, RP.with_rows(A, fs, exact), d)
        e.compute_pass(2); x.o.ComputePass(2)
        x.duals("float-valued rows"); x.bound("float-valued rows"); x.factor_bounds()
        x.m = A
        x.padding_untouched()
    _note("set_constants", "set_constants_check_kernel and the float-table branch of set_constants_kernel")


def test_pool_swap(p31):
    import torch
    import repool_cases as RP
    m = F.live("diff40")
    with Far(p31, m, ANISO) as x:
        e = x.e
        x.classes({"diff"})
        e.compute_pass(2); x.o.ComputePass(2)
        d = x.duals()
        built = e.schedules_built()
        for source, seed in (("host", 41), ("device", 42)):
            sh = RP.pool_of(m, seed)
            if source == "device":
                t = torch.from_numpy(sh).cuda(); torch.cuda.synchronize()
                e.upload_shared_pool(sh_dev=t.data_ptr())
            else:
                e.upload_shared_pool(sh)
            _restart_oracle(x, m.with_pool(sh), d)
            x.bound(source)
            e.compute_pass(2); x.o.ComputePass(2)
            d = x.duals(source)
            x.bound(source); x.factor_bounds(source)
            assert e.schedules_built() == built
        x.padding_untouched()
    _note("set_constants", "upload_shared_pool (the pool and its cells lie in an allocation of the engine, addressed relative to the far const base)")


# ---- prepared read-outs -----------------------------------------------------------------------------------------------------
# name -> (upload keywords, the model of the statement)
READOUT_MODELS = {name: ({}, lambda m: m) for name in ("dense8", "dense_v21", "big48", "potts16", "shared32", "diff40", "diff_shift40")}
READOUT_MODELS["dense32"] = ({"table_precision": "f32_round"}, lambda m: m.with_f32_tables())       # tab32: the tables read as floats


def _device_rows(x, call, n, stride):
    """``call(dst_dev, stride)`` into a torch tensor of n + 1 rows filled with the sentinel; the array afterwards"""
    import torch
    t = torch.from_numpy(np.full((n + 1) * stride, SENTINEL)).cuda()
    torch.cuda.synchronize()
    assert call(t.data_ptr(), stride) is None
    x.e.synchronize()
    return t.cpu().numpy().reshape(n + 1, stride)


def _check_rows(got_dev, want, what):
    """written entries equal; the padding of every row and the row behind the last are still the sentinel, bit for bit"""
    n = want.shape[0]
    written = ~np.isnan(want)
    assert np.array_equal(got_dev[:n][written], want[written]), what
    assert np.all(_bits(got_dev[:n][~written]) == _bits(SENTINEL)), what
    assert np.all(_bits(got_dev[n]) == _bits(SENTINEL)), what


def _readouts(bufs, name, family):
    import readout_cases as R
    kw, ref_of = READOUT_MODELS[name]
    m = F.live(name)
    ref = ref_of(m)
    us = np.asarray(R.unaries(m), np.int32)
    L = int(m.f_dim0[us].max())
    with Far(bufs, m, ANISO, oracle_of=lambda s: F.oracle_model(ref_of(s)), **kw) as x:
        e = x.e
        x.classes(F.LIVE[name][1])
        e.compute_pass(1); x.o.ComputePass(1)
        d = x.duals()
        stride = L + 3
        want = {"vectors": (R.vectors_np(m, d, us), R.vectors_np(m, d, us, stride=stride)),
                "beliefs": (R.beliefs_np(ref, d, us), R.beliefs_np(ref, d, us, stride=stride))}
        assert not np.array_equal(want["vectors"][0], want["beliefs"][0], equal_nan=True)
        primal = e.download_primal()
        assert np.array_equal(primal[us + x.n_pad, 0], m.f_dim0[us])                   # no label set: the label count
        for factors in (us + x.n_pad, None):        # None: every VECTOR factor — dense padding has none, so exactly the live unaries
            r = e.readout(factors)
            assert r.n == len(us) and r.max_labels == L
            for what, (host, dev) in want.items():
                call = getattr(r, what)
                assert np.array_equal(call(), host, equal_nan=True), (name, what)
                _check_rows(_device_rows(x, lambda p, s: call(p, s), r.n, stride), dev, (name, what))
            _check_labels(x, r, primal[us + x.n_pad, 0], name)
            r.close()
        e.synchronize()
        assert np.array_equal(bufs.dual_tail(), d)                  # a read-out reads only
        x.padding_untouched()
    _note(family, "readout_vectors_kernel<%d>" % (8 if L <= 8 else 16 if L <= 16 else 32 if L <= 32 else 64),
          "readout_beliefs_kernel<%d, 1>" % (4 if L <= 4 else 8 if L <= 8 else 16 if L <= 16 else 32 if L <= 32 else 64), "readout_labels_kernel")


@pytest.mark.parametrize("name", list(READOUT_MODELS))
def test_readouts(p31, name):
    _readouts(p31, name, "read-outs")


def test_readout_of_rounded_labels(p31):
    import readout_cases as R
    m = F.live("primal_dense8")
    us = np.asarray(R.unaries(m), np.int32)
    with Far(p31, m, ANISO) as x:
        r = x.e.readout(us + x.n_pad)
        x.e.compute_pass_and_primal(0); x.o.ComputePassAndPrimal(0)
        want = x.o.primal()[us, 0]
        assert np.all(want < m.f_dim0[us]) and np.array_equal(x.e.download_primal()[us + x.n_pad, 0], want)
        _check_labels(x, r, want, "after compute_pass_and_primal")
        r.close()
        x.duals()
        x.padding_untouched()


# ---- moving label windows ---------------------------------------------------------------------------------------------------
def _moved_shifts(m, us, delta):
    """the const array of ``m`` with every shift := shift + delta_left - delta_right (the unaries of a DIFF_SHIFT factor's two sides)"""
    row = {int(u): i for i, u in enumerate(us)}
    side = {(int(m.m_right[k]), int(m.mtypes[int(m.m_type[k])].param)): int(m.m_left[k]) for k in range(m.n_messages)}
    coff = m.const_offsets()
    const = np.array(m.const_data, np.float64, copy=True)
    for p in np.flatnonzero(m.f_kind == M.F_PAIRWISE_DIFF_SHIFT):
        dl, dr = (int(delta[row[side[(int(p), s)]]]) if side.get((int(p), s)) in row else 0 for s in (0, 1))
        const[coff[p] + 1] = float(min(max(M.diff_shift_int(const[coff[p] + 1]) + dl - dr, -(1 << 30)), 1 << 30))
    return const


def _moves(bufs, name, family):
    """four moves on one engine, two passes against the oracle on the moved model after each: deltas from the host, the way back from
    device memory, then with the unary costs of the old and the new window from the host and from device memory"""
    import torch
    import move_windows_cases as MW
    m = F.live(name)
    us = MW.unaries(m)
    L = int(m.f_dim0[us].max())
    delta = MW.deltas(m.f_dim0[us], L)
    assert {0, 1, -1, 63, -64, L - 1, -L, L + 7} <= set(delta.tolist())
    assert MW.has_hazard(m.f_dim0[us], delta) or L < 130
    stride = L + 6
    with Far(bufs, m, ANISO) as x:
        e = x.e
        x.classes({"diff"})
        ws = e.window_set(us + x.n_pad)
        assert ws.n == len(us) and ws.max_labels == L and ws.n_pairwise == int((m.f_kind == M.F_PAIRWISE_DIFF_SHIFT).sum())
        for n in (1, 2):
            e.compute_pass(n); x.o.ComputePass(n)
        d = x.duals("before the first move")
        built = e.schedules_built()
        for k, (dl, costs, dev) in enumerate(((delta, False, False), (-delta, False, True), (delta[::-1].copy(), True, False), (-delta[::-1], True, True))):
            co, cn = MW.cost_pair(x.m, us, dl, 12 + k, stride=stride) if costs else (None, None)
            keep = []
            if dev:
                keep = [torch.from_numpy(np.concatenate([dl, [1 << 30]]).astype(np.int32)).cuda()]
                if costs:
                    keep += [torch.from_numpy(co).cuda(), torch.from_numpy(cn).cuda()]
                torch.cuda.synchronize()
                ws.move(delta_dev=keep[0].data_ptr(), cost_dev=(keep[1].data_ptr(), keep[2].data_ptr()) if costs else None, stride=stride if costs else None)
                e.synchronize()
                assert np.array_equal(keep[0].cpu().numpy()[:-1], dl)
            else:
                ws.move(dl, cost_old=co, cost_new=cn)
            m2, d2 = M.move_windows(x.m, d, us, dl, co, cn)
            e.synchronize()
            got = bufs.dual_tail()
            assert not np.any(np.isnan(got)) and np.array_equal(got, d2), (name, k, int(np.sum(got != d2)))
            assert np.array_equal(m2.const_data, _moved_shifts(x.m, us, dl)) and not np.array_equal(m2.const_data, x.m.const_data), (name, k)
            assert np.array_equal(bufs.const_tail(), m2.const_data), (name, k)           # the shifts: a write into the borrowed const buffer
            assert bufs.const_padding_nonzero() == 0 and bufs.dual_padding_nonzero() == 0, (name, k)
            _restart_oracle(x, m2, d2)
            x.bound((name, k))
            e.compute_pass(2); x.o.ComputePass(2)
            d = x.duals((name, k))
            x.bound((name, k))
            assert e.schedules_built() == built                     # a move plans and builds nothing
        x.factor_bounds()
        ws.close()
        x.padding_untouched(const_tail=False)
        assert np.array_equal(bufs.const_tail(), x.m.const_data)
    _note(family, "move_windows_kernel (%d labels: %d of its 8 predicated blocks)" % (L, (L + 63) // 64), "move_shifts_kernel")


@pytest.mark.parametrize("name", ["diff_shift40", "diff_shift130"])
def test_moving_windows(p31, name):
    _moves(p31, name, "moving windows")


def test_a_window_set_next_to_a_dense_factor_is_refused(p31):
    m = F.live("diff_shift_mixed")
    dense = set(np.flatnonzero(m.f_kind == M.F_PAIRWISE_DENSE).tolist())
    u = next(int(m.m_left[k]) for k in range(m.n_messages) if int(m.m_right[k]) in dense)
    assert m.f_kind[u] == M.F_VECTOR
    with pytest.raises(M.WindowsUnsupported):
        M.window_links(m, [u])
    with Far(p31, m, ANISO) as x:
        x.e.compute_pass(2); x.o.ComputePass(2)
        d = x.duals()
        with pytest.raises(E.EngineError) as ei:
            x.e.window_set(np.array([u + x.n_pad], np.int32))
        assert ei.value.code == UNSUPPORTED and "factor %d " % (u + x.n_pad) in str(ei.value), str(ei.value)
        x.e.synchronize()
        assert p31.dual_tail().tobytes() == d.tobytes()
        x.padding_untouched()                                       # constants and both paddings bitwise as before


# ---- labeling lists whose left factor has several labelings ------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["level loop", "chain tickets"])
@pytest.mark.parametrize("name", list(F.LABELING_NL))
def test_labeling_lists_with_several_left_labelings(p31, name, engine, monkeypatch):
    import labeling_cases as LC
    c = LC.CASES[F.LABELING_NL[name]]
    assert c.fam.nl > 1
    monkeypatch.delenv("LPMP_NO_CHAIN", raising=False)
    for k in ("LPMP_NO_LEVEL_LOOP", "LPMP_CHAIN_ALL", "LPMP_CHAIN_MIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(LC.ENGINES)[engine].items():
        monkeypatch.setenv(k, v)
    m = F.live(name)
    for mode in MODES:
        with Far(p31, m, mode) as x:
            LC.assert_path(x.e.plan, c, engine)                     # on the FAR plan, before anything runs
            if engine == "level loop" and c.fam.cls == "small":
                reached = {b for d in (M.FORWARD, M.BACKWARD, -1) for md in MODES for b, n in LC.bodies(x.e.plan, d, md).items() if n > 0}
                assert {"paired staged", "staged"} <= reached, reached
                _note("labeling lists, nl > 1", "level loop of class small, bodies %s (nl = %d)" % (sorted(reached), c.fam.nl))
            else:
                _note("labeling lists, nl > 1", "%s of class %s (nl = %d)" % (engine, c.fam.cls, c.fam.nl))
            x.bound("upload")
            for what, n in LC.CALLS:
                LC.call(x.e, what, n); LC.call(x.o, what, n)
                x.duals((what, n))
                x.bound((what, n))
            x.factor_bounds()
            x.padding_untouched()


# ---- placement P32: an unsigned 32-bit truncation shows here, not at P31 ----------------------------------------------------
class TestP32:
    @pytest.mark.parametrize("name", F.P32_MODELS)
    def test_first_three_families_past_two_to_the_32(self, p32, name):
        assert p32.pad_c >= 2**32 and p32.pad_d >= 2**32
        kernel = {**PACKED_DENSE, **PACKED_POTTS, **STREAMING}[name]
        _run(p32, name, "P32 " + name, kernel=kernel)

    def test_diff_shift_sweep(self, p32):
        assert p32.pad_c >= 2**32 and p32.pad_d >= 2**32
        _diff_shift_sweep(p32, "diff_shift40", "P32 diff shift")

    @pytest.mark.parametrize("engine", ["default", "no_peer_minima", "ahead0"])
    def test_joined_passes_with_and_without_peer_minima(self, p32, engine, monkeypatch, capfd):
        _joined_passes(p32, "joined_dense32", engine, monkeypatch, capfd)

    @pytest.mark.parametrize("name", list(READOUT_MODELS))
    def test_readouts(self, p32, name):
        _readouts(p32, name, "P32 read-outs")

    @pytest.mark.parametrize("name", ["diff_shift40", "diff_shift130"])
    def test_moving_windows(self, p32, name):
        _moves(p32, name, "P32 moving windows")
