"""Every kernel family at constant and dual offsets past 2^31 elements (placement P31; the packed dense, packed Potts and streaming
dense families past 2^32 as well, P32).  tests/far_offset_cases.py puts tens of thousands of isolated, all-zero padding factors in
front of a small live model; the costs live in two borrowed device tensors of about 16 GiB (32 GiB) each, the live part at their
tails.  The far engine never moves its duals through the host: after ``synchronize()`` the tail of the borrowed dual tensor is
compared with the oracle's duals of the SMALL model, bit for bit, and both padding regions must still be all +0.0.

Tolerances are those of tests/test_diff_tables_gpu.py.  The kernel class is asserted before anything runs.  Whether the planner
hands out the right offsets is tests/test_far_offsets_host.py; this module is about the kernels' index arithmetic."""
import dataclasses
import json

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S
from oracle.binding import Oracle

import far_offset_cases as F
import recost_cases as RC

pytestmark = pytest.mark.gpu

LB_RTOL = 1e-5
FLB_ATOL = 1e-12
ANISO, UNIFORM = M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM
MODES = (ANISO, UNIFORM)
SLACK = 8 * F.GIB
_mem = {"free0": None, "min_free": None, "ran": set(), "kernels": {}}


def _sample_memory():
    import torch
    free = torch.cuda.mem_get_info()[0]
    if _mem["free0"] is None:
        _mem["free0"] = free
    _mem["min_free"] = free if _mem["min_free"] is None else min(_mem["min_free"], free)


def _buffers(placement, kind="dense"):
    import torch
    _sample_memory()
    need, free = F.FarBuffers.bytes_needed(placement, kind), torch.cuda.mem_get_info()[0]
    if free < need + SLACK:
        pytest.skip("placement %s (%s padding) needs %.1f GiB + 8 GiB, the device reports %.1f GiB free" % (placement, kind, need / F.GIB, free / F.GIB))
    return F.FarBuffers(placement, kind)


def _release(b):
    import torch
    b.const = b.dual = None
    torch.cuda.empty_cache()


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


class Far:
    """an engine on pad_front(m) over the borrowed buffers, and the oracle on the small model"""

    def __init__(self, bufs, m, mode, oracle_of=F.oracle_model, const=None, dual=None, **upload_kw):
        self.bufs, self.m, self.n_pad = bufs, m, bufs.n_pad
        self.far = F.pad_front(m, bufs.n_pad, bufs.kind)
        assert int(self.far.const_offsets()[self.n_pad]) == bufs.pad_c and int(self.far.dual_offsets()[self.n_pad]) == bufs.pad_d
        assert bufs.pad_d >= 2**31 and (bufs.kind == "vector" or bufs.pad_c >= 2**31)
        cp, dp = bufs.load(m, const, dual)
        assert bufs.dual_padding_nonzero() == 0
        self.o = Oracle(oracle_of(m)); self.o.set_reparametrization(mode)
        self.e = E.Engine(0)
        try:
            self.e.upload(self.far, const_dev=cp, dual_dev=dp, keep=(bufs.const, bufs.dual), **upload_kw)
            self.e.set_reparametrization(mode)
        except BaseException:
            self.e.close()
            raise
        self.mode = mode
        _mem["ran"].add(bufs.placement + " " + bufs.kind)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _sample_memory()
        self.e.close()
        self.bufs.reset()                    # the used tails go back to zero after every engine

    def classes(self, only=None, some=None):
        """asserted BEFORE anything runs, so that a fallback cannot stand in"""
        for d in (0, 1):
            c = self.e.plan.schedule_classes(d, self.mode)
            if only is not None:
                assert set(c) == set(only), (c, only)
            if some is not None and d == 1:
                assert set(c) & set(some), (c, some)

    def bound(self, what=""):
        lb, lbo = self.e.lower_bound(), self.o.LowerBound()
        assert np.isfinite(lb) and abs(lb - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (what, lb, lbo)

    def duals(self, what=""):
        """the tail of the borrowed buffer against the oracle; never download_duals()"""
        self.e.synchronize()
        d, do = self.bufs.dual_tail(), self.o.duals()
        assert not np.any(np.isnan(d)), what
        assert np.array_equal(d, do), (what, float(np.max(np.abs(d - do))))
        return d

    def factor_bounds(self, what=""):
        flb = self.e.factor_lower_bounds()
        assert flb.shape[0] == self.far.n_factors
        assert np.all(flb[:self.n_pad] == 0.0), what
        ref = np.array([self.o.factor_lower_bound(f) for f in range(self.m.n_factors)])
        assert np.max(np.abs(flb[self.n_pad:] - ref)) <= FLB_ATOL, (what, float(np.max(np.abs(flb[self.n_pad:] - ref))))

    def padding_untouched(self, const_tail=True):
        self.e.synchronize()
        assert self.bufs.dual_padding_nonzero() == 0
        assert self.bufs.const_padding_nonzero() == 0
        if const_tail:
            assert np.array_equal(self.bufs.const_tail(), self.m.const_data)     # the constants are read-only

    def timed_passes(self, n, family):
        self.e.enable_kernel_timing(True); self.e.reset_kernel_timing()
        self.e.compute_pass(n); self.o.ComputePass(n)
        kt = self.e.kernel_timing()
        self.e.enable_kernel_timing(False)
        names = sorted(v["kernel"] for v in kt.values())
        _mem["kernels"].setdefault(family, [])
        for k in names:
            if k not in _mem["kernels"][family]:
                _mem["kernels"][family].append(k)
        return kt

    def standard(self, family):
        """3 single passes with the bound after each, then compute_pass(2) (timed: the kernel that ran), duals, per-factor bounds"""
        self.bound("upload")
        for k in range(3):
            self.e.compute_pass(1); self.o.ComputePass(1)
            self.bound(k)
        kt = self.timed_passes(2, family)
        self.bound("after 2 more")
        self.duals()
        self.factor_bounds()
        self.padding_untouched()
        return kt


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
    monkeypatch.setenv("LPMP_ROT_BANDS", "8"); monkeypatch.setenv("LPMP_ROT_LAG", "2"); monkeypatch.setenv("LPMP_ROT_DEPTH", "4")
    with Far(p31, F.live(name), ANISO) as x:
        x.classes(F.LIVE[name][1])
        assert x.e.plan.pass_rotates(ANISO)
        for n in (1, 5, 2):
            kt = x.timed_passes(n, "joined passes")
            assert all(v["kernel"].startswith("chain_") and v["chain_launches"] == 1 for v in kt.values()), kt
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


# ---- rows layout ------------------------------------------------------------------------------------------------------------
class TestRowsLayout:
    def test_rows_layout_behind_vector_padding(self, p31_vector):
        m = F.live("dense8")
        for mode in MODES:
            with Far(p31_vector, m, mode, rows_layout=True) as x:
                assert x.e.rows_layout
                x.classes({"dense8"})
                x.standard("rows layout")       # duals(): after synchronize() the packed tail holds the oracle's duals


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


# ---- placement P32: an unsigned 32-bit truncation shows here, not at P31 ----------------------------------------------------
class TestP32:
    @pytest.mark.parametrize("name", F.P32_MODELS)
    def test_first_three_families_past_two_to_the_32(self, p32, name):
        assert p32.pad_c >= 2**32 and p32.pad_d >= 2**32
        kernel = {**PACKED_DENSE, **PACKED_POTTS, **STREAMING}[name]
        _run(p32, name, "P32 " + name, kernel=kernel)
