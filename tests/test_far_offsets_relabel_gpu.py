"""The kernels that relabel and keep the primal state, and the newer sweep forms, at constant and dual offsets past 2^31 elements
(placement P31; a choice of them past 2^32 as well, P32): path moves, forest moves, labels written in and carried through a window
move, the two scalars written into device memory, and the banded form of shifted difference-indexed factors.  The second module of
the far-offset suite: tests/test_far_offsets_gpu.py has the sweep families and the calls around them, tests/far_offset_gpu.py what
both share, tests/far_offset_cases.py the padding and the live models, tests/test_far_offsets_host.py the planner's side and the
conditions on the inputs that keep every test here from passing vacuously.

Every test takes the code path of its near test (tests/test_path_moves_gpu.py, test_forest_moves_gpu.py, test_primal_state_gpu.py,
test_diff_shift_band_gpu.py) with the same numpy statement or oracle as the yardstick, on the SMALL model; what is new is that the
records hold far offsets and factor numbers beyond the padding.  The duals are read from the tail of the borrowed tensor after
``synchronize()``, never through the host; labels are ``np.array_equal``, doubles compared by their bits."""
import json

import numpy as np
import pytest

from lp_mp_amd import model as M

import far_offset_cases as F
from far_offset_gpu import LB_RTOL, Far, _buffers, _mem, _note, _release, _restart_oracle, _sample_memory, _timed

pytestmark = pytest.mark.gpu

ANISO, UNIFORM = M.REPAM_ANISOTROPIC, M.REPAM_UNIFORM
MODES = (ANISO, UNIFORM)
NAN_BITS = 0x7FF8_0000_DEAD_BEEF                  # the sentinel around a destination: a NaN with a payload (tests/test_primal_state_gpu.py)
PATH_WAVE_MAX = 64                                # above it a path, or a tree node with its parent, takes a workgroup (csrc/kernels.hpp)


@pytest.fixture(scope="module")
def p31():
    b = _buffers("P31")
    yield b
    _release(b)
    print("\nfar offsets, relabel: placements that ran: %s; peak device memory in use beyond the start of the far modules: %.1f GiB"
          % (sorted(_mem["ran"]), (_mem["free0"] - _mem["min_free"]) / F.GIB))
    print("far offsets: kernels per family: " + json.dumps(_mem["kernels"], sort_keys=True))


@pytest.fixture(scope="class")
def p32():
    b = _buffers("P32")
    yield b
    _release(b)


@pytest.fixture(autouse=True)
def _memory_after_every_test():
    yield
    _sample_memory()


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _same(a, b):
    return _bits(a).tobytes() == _bits(b).tobytes()


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _differ(got, want):
    bad = np.argwhere(got != want)
    return bad[:8].tolist(), got[bad[:8, 0]].tolist(), want[bad[:8, 0]].tolist()


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


def _far_primal(x, small):
    """the far engine's label array with the small model's ``small`` behind the padding rows as they are: (array, padding rows)"""
    p = x.e.download_primal()
    assert p.shape == (x.far.n_factors, 2)
    pad = p[:x.n_pad].copy()
    p[x.n_pad:] = small
    return p, pad


def _labels_are(x, want, pad, what):
    got = x.e.download_primal()
    assert np.array_equal(got[x.n_pad:], want), (what,) + _differ(got[x.n_pad:], want)
    assert np.array_equal(got[:x.n_pad], pad), (what, "padding rows")
    return got


# ---- path and forest moves ------------------------------------------------------------------------------------------------------
def _forms(kind, m, groups):
    """the kernels the planner's rule gives these groups (csrc/prepared.cpp): a path by its widest node, a tree node by itself and
    its parent; moves are not timed by kernel_timing"""
    d = lambda u: int(m.f_dim0[int(u)])
    out = set()
    if kind == "path":
        for g in groups:
            for p in g:
                out.add("path_moves_kernel<%d>" % (256 if max(d(u) for u in p) > PATH_WAVE_MAX else 64))
    else:
        for un, par in groups:
            for u, q in zip(un, par):
                out.add("forest_up_kernel<%d>" % (256 if max(d(u), d(q) if q != -1 else 0) > PATH_WAVE_MAX else 64))
                if q != -1:
                    out.add("forest_down_kernel")
    return sorted(out)


def _relabel(bufs, kind, name, after=None):
    """tests/test_path_moves_gpu.py / test_forest_moves_gpu.py ``_check_moves`` behind the padding: after every group of every round
    (one prepared set per group, moved in turn), then the whole move through one set; the padding rows of the label array, both
    tails and both paddings are what they were.  ``after(x, labels, duals)``: more calls on the engine the move left"""
    c = F.RELABEL[kind][name]
    m, groups, ref = F.relabel_case(kind, name)
    kw = dict(c.kw)
    with Far(bufs, m, ANISO, oracle_of=None, dual=F.relabel_random_duals(kind, name), **kw) as x:
        e, n_pad = x.e, x.n_pad
        if kw:
            assert e.table_precision() == kw["table_precision"]
        if c.passes:
            e.compute_pass(c.passes)
        e.synchronize()
        duals, consts = bufs.dual_tail(), bufs.const_tail()
        assert not np.any(np.isnan(duals)), name
        assert c.passes or np.array_equal(duals, F.relabel_random_duals(kind, name))
        start = F.relabel_start(kind, name)
        trace = []
        want = F.relabel_reference(kind, name, duals, start, trace=trace)
        members = F.relabel_members(kind, groups)
        assert not np.array_equal(trace[len(groups) - 1][members, 0], start[members, 0]), "the first round moves no label: the test would pass vacuously"
        base, pad = _far_primal(x, start)
        make = e.path_set if kind == "path" else e.forest_set
        far = F.far_groups(kind, groups, n_pad)
        e.upload_primal(base)
        sets = [make([g]) for g in far]
        for i, t in enumerate(trace):
            sets[i % len(groups)].move(1)
            _labels_are(x, t, pad, (name, "round %d group %d" % divmod(i, len(groups))))
        for s in sets:
            s.close()
        e.upload_primal(base)
        s = make(far)
        assert s.n_groups == len(groups)
        if (kind, name) == ("path", "rect_both_forms"):     # both forms in one group, one- and two-byte back-pointers in one path
            assert s.scratch_bytes == (40 + 9 + 70) + (300 + 7 * 2 + (257 + 1)) and s.longest == 4
        if (kind, name) == ("path", "length300"):
            assert s.longest == 300
        s.move(F.RELABEL_ROUNDS)
        got = _labels_are(x, want, pad, (name, "whole move"))
        s.close()
        e.synchronize()
        assert bufs.dual_tail().tobytes() == duals.tobytes() and bufs.const_tail().tobytes() == consts.tobytes(), name      # a move reads only
        x.padding_untouched()
        if after is not None:
            after(x, got, duals)
    _note("P32 %s moves" % kind if bufs.placement == "P32" else "%s moves" % kind, *_forms(kind, m, groups))


@pytest.mark.parametrize("name", list(F.PATH_CASES))
def test_path_moves(p31, name):
    _relabel(p31, "path", name)


@pytest.mark.parametrize("name", list(F.FOREST_CASES))
def test_forest_moves(p31, name):
    _relabel(p31, "forest", name)


# ---- labels written in ------------------------------------------------------------------------------------------------------------
def _set_labels(bufs, name, family):
    """a read-out over the live unaries in a permuted order; host labels with unset entries, then device labels with strays below 0
    and at or above the label count, which are stored as unset where they are read"""
    import primal_state_cases as PS
    m = F.live(name)
    u = PS.unaries(m)
    f = np.random.default_rng(len(u)).permutation(u).astype(np.int32)
    d = m.f_dim0[f].astype(np.int64)
    rng = np.random.default_rng(23)
    with Far(bufs, m, ANISO, oracle_of=None) as x:
        e, n_pad = x.e, x.n_pad
        e.compute_pass(1)
        e.synchronize()
        duals = bufs.dual_tail()
        small = PS.random_primal(m, 1, unset_every=7)
        base, pad = _far_primal(x, small)
        e.upload_primal(base)
        r = e.readout(f + n_pad)
        assert r.n == len(f)
        src = rng.integers(0, d).astype(np.int32)
        src[::5] = d[::5]                                       # unset
        keep = src.copy()
        r.set_labels(src)
        assert np.array_equal(src, keep) and np.array_equal(r.labels(), keep)
        small = PS.set_labels_reference(m, small, f, keep)
        _labels_are(x, small, pad, (name, "host"))
        src = rng.integers(0, d).astype(np.int32)
        at = np.arange(1, 25, 4)                                # six strays: below 0, at the label count and above it
        src[at] = [-1, -(1 << 31), (1 << 31) - 1, d[at[3]], d[at[4]] + 1, d[at[5]] + 7]
        assert np.any(src < 0) and np.any(src == d) and np.any(src > d) and np.any((src >= 0) & (src < d))
        keep = src.copy()
        t = _dev(np.concatenate([src, [-(1 << 31)]]).astype(np.int32))
        r.set_labels(src_dev=t.data_ptr())
        e.synchronize()
        assert np.array_equal(t.cpu().numpy()[:-1], keep)
        stored = np.where((keep >= 0) & (keep < d), keep, d)
        assert np.array_equal(r.labels(), stored)
        small = PS.set_labels_reference(m, small, f, keep)
        _labels_are(x, small, pad, (name, "device"))
        r.close()
        e.synchronize()
        assert bufs.dual_tail().tobytes() == duals.tobytes()
        x.padding_untouched()
    _note(family, "set_labels_kernel (host and device labels), primal_propagate_kernel")


@pytest.mark.parametrize("name", F.SET_LABEL_MODELS)
def test_set_labels(p31, name):
    _set_labels(p31, name, "labels written in")


# ---- window moves: carried labels, and the shift word of a banded cell ---------------------------------------------------------------
def _window_moves(bufs, name, family, carry, more=(), feasible=True):
    """the four moves of tests/test_far_offsets_gpu.py ``_moves`` on one engine — deltas from the host, the way back from device
    memory, then with the unary costs of the old and the new window from the host and from device memory — with two passes against
    the oracle on the moved model after each, checked as there.  ``carry``: every move through lpmp_move_windows_carry on a labelling
    uploaded before it; the labels afterwards are ``model.move_labels``.  ``more``: moves run behind the four.  ``feasible=False``: a
    move may leave the model without a finite labelling (a vector with +inf tails whose band leaves the diagonal; the moved duals
    are finite still).  Then the engine's bound must be the oracle's +inf, and no pass runs on that state: passes on it compute
    inf - inf on either side, and NaN is the engine's mark of a stale bound, so there is nothing an oracle could say about them.
    Prints which shifted kernel the passes ran"""
    import torch
    import move_windows_cases as MW
    from test_far_offsets_gpu import _moved_shifts
    m = F.live(name)
    us, L, moves = F.window_moves(name)
    assert {0, 1, -1, 63, -64, L - 1, -L, L + 7} <= set(moves[0][0].tolist())
    assert MW.has_hazard(m.f_dim0[us], moves[0][0]) or L < 130
    stride = L + 6
    d_us = m.f_dim0[us]
    with Far(bufs, m, ANISO) as x:
        e = x.e
        x.classes({"diff"})
        ws = e.window_set(us + x.n_pad)
        assert ws.n == len(us) and ws.max_labels == L and ws.n_pairwise == int((m.f_kind == M.F_PAIRWISE_DIFF_SHIFT).sum())
        for n in (1, 2):
            e.compute_pass(n); x.o.ComputePass(n)
        d = x.duals("before the first move")
        built = e.schedules_built()
        ran_passes = []
        for k, (dl, costs, dev, labels) in enumerate(list(moves) + list(more)):
            co, cn = MW.cost_pair(x.m, us, dl, 12 + k, stride=stride) if costs else (None, None)
            kw = dict(carry_labels=True) if carry else {}
            if carry:
                base, pad = _far_primal(x, labels)
                e.upload_primal(base)
            if dev:
                keep = [torch.from_numpy(np.concatenate([dl, [1 << 30]]).astype(np.int32)).cuda()]
                if costs:
                    keep += [torch.from_numpy(co).cuda(), torch.from_numpy(cn).cuda()]
                torch.cuda.synchronize()
                ws.move(delta_dev=keep[0].data_ptr(), cost_dev=(keep[1].data_ptr(), keep[2].data_ptr()) if costs else None, stride=stride if costs else None, **kw)
                e.synchronize()
                assert np.array_equal(keep[0].cpu().numpy()[:-1], dl)
            else:
                ws.move(dl, cost_old=co, cost_new=cn, **kw)
            m2, d2 = M.move_windows(x.m, d, us, dl, co, cn)
            e.synchronize()
            got = bufs.dual_tail()
            assert not np.any(np.isnan(got)) and np.array_equal(got, d2), (name, k, int(np.sum(got != d2)))
            assert np.array_equal(m2.const_data, _moved_shifts(x.m, us, dl)) and not np.array_equal(m2.const_data, x.m.const_data), (name, k)
            assert np.array_equal(bufs.const_tail(), m2.const_data), (name, k)           # the shifts: a write into the borrowed const buffer
            assert bufs.const_padding_nonzero() == 0 and bufs.dual_padding_nonzero() == 0, (name, k)
            if carry:
                want = M.move_labels(labels, m, us, dl)
                got = _labels_are(x, want, pad, (name, k, "carried labels"))
                unset = labels[us, 0] == d_us
                assert unset.any() and np.array_equal(got[us + x.n_pad, 0] == d_us, unset), (name, k)      # an unset slot stays unset
            _restart_oracle(x, m2, d2)
            d = d2
            if not feasible and x.o.LowerBound() == np.inf:
                assert e.lower_bound() == np.inf, (name, k)         # the bound kernels read the shift words the move wrote
                print("%s, move %d: no finite labelling is left (bound +inf on the engine and the oracle); no pass on this state" % (name, k))
                continue
            ran_passes.append(k)
            x.bound((name, k))
            kt = _timed(x, lambda: (e.compute_pass(2), x.o.ComputePass(2)), family)
            print("%s, move %d: the passes after it ran %d launches, %d of them shifted, %d of them banded" %
                  (name, k, kt["diff"]["launches"], kt["diff"]["shift_launches"], kt["diff"]["shift_band_launches"]))
            d = x.duals((name, k))
            x.bound((name, k))
            assert e.schedules_built() == built                     # a move plans and builds nothing
        assert feasible or set(range(len(moves), len(moves) + len(more))) <= set(ran_passes), ran_passes
        x.factor_bounds()
        ws.close()
        x.padding_untouched(const_tail=False)
        assert np.array_equal(bufs.const_tail(), x.m.const_data)
    _note(family, "move_windows_kernel (%d labels)" % L, "move_shifts_kernel", *(["carry_labels_kernel (host and device deltas)"] if carry else []))


@pytest.mark.parametrize("name", F.CARRY_MODELS)
def test_labels_carried_through_window_moves(p31, name):
    _window_moves(p31, name, "carried labels", carry=True)


# ---- the scalars in device memory ------------------------------------------------------------------------------------------------
def _bound_in_device_memory(bufs, name, family):
    """the procedure of tests/test_far_offsets_gpu.py test_full_and_list_bound_kernels with the bound written into device memory: a full
    recompute after invalidate_lower_bounds, then the send-only custom pass that leaves some bounds stale — once with the host call,
    whose counter says how many (the pass marks the same bounds whatever the duals), once more with the device call, whose list
    kernel reads the count on the device.  Each device value has the bits of the host call made right after it"""
    from test_far_offsets_gpu import send_only_updates
    m = F.live(name)
    cell = Cell()
    with Far(bufs, m, ANISO) as x:
        e, nf = x.e, x.far.n_factors

        def both(what):
            e.lower_bound(cell.ptr)
            got = cell.read(e)
            host, lbo = e.lower_bound(), x.o.LowerBound()
            assert np.isfinite(host) and _same(got, host), (name, what, got, host)
            assert abs(got - lbo) <= LB_RTOL * max(1.0, abs(lbo)), (name, what, got, lbo)

        e.compute_pass(1); x.o.ComputePass(1)
        e.invalidate_lower_bounds()
        both("full")                                       # dense_lb_kernel / factor_lb_kernel over every factor, sum_stage, sum_final_kernel
        assert e.lower_bound_recomputed() == 0             # (the host call found every bound fresh: the device call had recomputed all)
        rows = send_only_updates(x.o, ANISO)
        assert len(rows[0]) > 0
        e.compute_pass_custom(rows[0] + x.n_pad, *rows[1:]); x.o.compute_pass_custom(*rows)
        x.bound("list, host")
        n = e.lower_bound_recomputed()
        print(name, "bounds the custom pass leaves stale:", n, "of", nf)
        assert 0 < n <= nf // 8
        e.compute_pass_custom(rows[0] + x.n_pad, *rows[1:]); x.o.compute_pass_custom(*rows)
        both("list, device")                               # lb_collect_stale_kernel, factor_lb_list_dev_kernel on n entries
        assert e.lower_bound_recomputed() == 0             # (nothing left for the host call: the device list was the stale set)
        x.factor_bounds("list")
        x.duals()
        x.padding_untouched()
    _note(family, "lb_collect_stale_kernel", "factor_lb_list_dev_kernel", "sum_final_kernel")


@pytest.mark.parametrize("name", F.SCALAR_MODELS)
def test_lower_bound_in_device_memory(p31, name):
    _bound_in_device_memory(p31, name, "scalars in device memory")


def test_primal_cost_in_device_memory_after_a_path_move(p31):
    """the path move of test_path_moves[dense13], then lpmp_evaluate_primal_dev with the padding labelled (0, 0) at cost 0.0 each (no
    move labels an isolated factor; unset it would make the sum +inf, as in test_primal_rounding of tests/test_far_offsets_gpu.py)"""
    import primal_state_cases as PS
    cell = Cell()

    def after(x, labels, duals):
        e, n_pad, m = x.e, x.n_pad, x.m
        p = labels.copy()
        p[:n_pad] = 0
        e.upload_primal(p)
        assert e.check_primal_consistency()
        e.evaluate_primal(cell.ptr)
        got = cell.read(e)
        host, want = e.evaluate_primal(), PS.energy(m, duals, p[n_pad:])
        assert np.isfinite(host) and _same(got, host), (got, host)
        assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (got, want)
        stray = p.copy()
        pw = int(np.flatnonzero(m.f_kind != M.F_VECTOR)[5])
        stray[n_pad + pw, 1] = (stray[n_pad + pw, 1] + 1) % int(m.f_dim1[pw])
        e.upload_primal(stray)
        e.evaluate_primal(cell.ptr)
        assert cell.read(e) == np.inf and e.evaluate_primal() == np.inf
        e.upload_primal(p)                                          # ... and back
        e.evaluate_primal(cell.ptr)
        assert _same(cell.read(e), host)
        x.padding_untouched()

    _relabel(p31, "path", "dense13", after=after)
    _note("scalars in device memory", "primal_cost_kernel", "sum_final_kernel")


# ---- the banded form of shifted difference-indexed factors -----------------------------------------------------------------------
def _banded_sweep(bufs, name, family):
    m = F.live(name)
    for mode in MODES:
        with Far(bufs, m, mode) as x:
            x.classes({"diff"})
            for d in (0, 1):                 # on the FAR plan, before anything runs: every shifted launch is banded
                i = x.e.plan.diff_shift_band_info(d, mode)
                assert i["shift_band_launches"] == i["shift_launches"] > 0, (name, mode, d, i)
                assert x.e.plan.diff_band_info(d, mode)["band_launches"] == 0
            kt = _timed(x, lambda: (x.e.forward_pass(), x.o.ComputeForwardPass()), family)
            assert set(kt) == {"diff"} and kt["diff"]["kernel"] == "sweep_diff_shift_kernel", kt
            assert kt["diff"]["shift_band_launches"] == kt["diff"]["launches"] > 0 and kt["diff"]["band_launches"] == 0, kt
            x.duals("forward")
            kt = x.standard(family)
            assert kt["diff"]["shift_band_launches"] == kt["diff"]["launches"] > 0, kt
    _note(family, "sweep_diff_shift_band_kernel (every launch: shift_band_launches == launches, %d labels)" % int(m.f_dim0.max()))


@pytest.mark.parametrize("name", F.DIFF_SHIFT_BAND_MODELS)
def test_banded_diff_shift_sweep(p31, name):
    _banded_sweep(p31, name, "diff shift banded")


def test_a_move_rewrites_the_shift_of_a_banded_cell(p31):
    """the next pass must use the shift word a move wrote into the borrowed const buffer: the oracle on ``model.move_windows``' model
    says what it computes.  Whether a pass runs banded follows the vectors and the label counts, not the shifts (tests/
    diff_shift_band_cases.py ``banded``), so the moved model is expected on the banded kernel still; only the oracle equality is
    asserted.  The model has a vector with +inf tails, its band kept on the diagonal; the deltas of the four moves — up to L + 7
    labels between neighbours — push it off, and the moved model has no finite labelling until the windows are back (tests/
    test_far_offsets_host.py says after which moves).  There the bound is compared (+inf on both sides) and no pass runs.  Two more
    moves change the shift of every cell by one and keep the model feasible: the passes behind them run on rewritten shift words"""
    _window_moves(p31, "diff_shift_band40", "diff shift banded, moved windows", carry=False, more=F.checkerboard_moves("diff_shift_band40"), feasible=False)


# ---- placement P32: an unsigned 32-bit truncation shows here, not at P31 ----------------------------------------------------------
class TestP32:
    @pytest.mark.parametrize("name", F.P32_RELABEL["path"])
    def test_path_moves(self, p32, name):
        assert p32.pad_c >= 2**32 and p32.pad_d >= 2**32
        _relabel(p32, "path", name)

    @pytest.mark.parametrize("name", F.P32_RELABEL["forest"])
    def test_forest_moves(self, p32, name):
        _relabel(p32, "forest", name)

    def test_set_labels(self, p32):
        _set_labels(p32, "primal_dense8", "P32 labels written in")

    def test_lower_bound_in_device_memory(self, p32):
        _bound_in_device_memory(p32, "dense8", "P32 scalars in device memory")

    def test_banded_diff_shift_sweep(self, p32):
        assert p32.pad_c >= 2**32 and p32.pad_d >= 2**32
        _banded_sweep(p32, "diff_shift_band40", "P32 diff shift banded")
