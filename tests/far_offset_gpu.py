"""What the far-offset GPU modules share (tests/test_far_offsets_gpu.py, tests/test_far_offsets_relabel_gpu.py): the borrowed
buffers of a placement, the ``Far`` engine on ``pad_front(m)`` over them with the oracle on the small model, and the notes for the
closing printout.  A plain module: no fixtures live here — each test module keeps its own, so the two never hold their buffers at
the same time — and nothing here is collected."""
import dataclasses

import numpy as np
import pytest

from lp_mp_amd import engine as E
from oracle.binding import Oracle

import far_offset_cases as F

LB_RTOL = 1e-5
FLB_ATOL = 1e-12
SLACK = 8 * F.GIB
SENTINEL_I32 = np.int32(-0x5EADBEF)
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


class Far:
    """an engine on pad_front(m) over the borrowed buffers, and the oracle on the small model"""

    def __init__(self, bufs, m, mode, oracle_of=F.oracle_model, const=None, dual=None, **upload_kw):
        self.bufs, self.m, self.n_pad = bufs, m, bufs.n_pad
        self.far = F.pad_front(m, bufs.n_pad, bufs.kind)
        assert int(self.far.const_offsets()[self.n_pad]) == bufs.pad_c and int(self.far.dual_offsets()[self.n_pad]) == bufs.pad_d
        assert bufs.pad_d >= 2**31 and (bufs.kind == "vector" or bufs.pad_c >= 2**31)
        cp, dp = bufs.load(m, const, dual)
        assert bufs.dual_padding_nonzero() == 0
        self.o = None                        # (oracle_of=None: the caller compares with a trajectory computed once)
        if oracle_of is not None:
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


def _note(family, *kernels):
    """kernels that kernel_timing does not name, for the closing printout"""
    have = _mem["kernels"].setdefault(family, [])
    have += [k for k in kernels if k not in have]


def _timed(x, call, family):
    x.e.enable_kernel_timing(True); x.e.reset_kernel_timing()
    call()
    kt = x.e.kernel_timing()
    x.e.enable_kernel_timing(False)
    _note(family, *sorted(v["kernel"] for v in kt.values()))
    return kt


def _restart_oracle(x, m, duals):
    """the oracle again, on model ``m`` (same structure) with the packed ``duals``: after a call that changed constants or moved duals"""
    x.m = m
    x.o = Oracle(dataclasses.replace(F.oracle_model(m), dual_data=np.array(duals, np.float64, copy=True), _keep=[]))
    x.o.set_reparametrization(x.mode)


def _check_labels(x, r, want, what):
    import torch
    assert np.array_equal(r.labels(), want), what
    t = torch.from_numpy(np.full(r.n + 1, SENTINEL_I32, np.int32)).cuda()
    torch.cuda.synchronize()
    assert r.labels(t.data_ptr()) is None
    x.e.synchronize()
    got = t.cpu().numpy()
    assert np.array_equal(got[:r.n], want) and got[r.n] == SENTINEL_I32, what
