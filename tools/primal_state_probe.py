#!/usr/bin/env python3
"""Times what the host round trip of the two scalars costs, and what a start labelling costs to bring in.  GPU only: there is no CPU
path, a missing device is an error.

    python tools/primal_state_probe.py --grid 1024 --labels 32 --iters 40 --repeat 3
    LPMP_ENGINE_SO=/path/to/an/older/liblpmp_engine.so python tools/primal_state_probe.py --grid 1024 --iters 40 --repeat 3

On the headline grid (bench.py's C3: dense tables, colour-major order, costs generated on the device) it times
  scalars   the solver loop  compute_pass(1) + bound,  ITERS iterations, one host synchronisation at the end, with
              host   lpmp_lower_bound     (a copy of the partial sums to pinned memory and a stream synchronisation per iteration)
              dev    lpmp_lower_bound_dev (one double into device memory, nothing waits)
            each with passes that run ahead off (speculation 0) and on (speculation 8); ms per iteration, REPEAT repetitions
            alternating.  A library without the device call (LPMP_ENGINE_SO: the parent commit's, for the baseline of the host call)
            runs the host rows only.  The variants run one after the other on one engine, so the last bound of each (reported
            for the record) is that of a later pass; on one state the two calls are compared at the end (bound_bits_equal), and
            the bound alone is timed there, 200 calls between two synchronisations.
  labels    one round of path moves over the rows and columns from a random labelling that comes in through
              set_labels     Readout.set_labels from a device array (no host synchronisation) + PathSet.move(1)
              upload_primal  Engine.upload_primal of the [2 * n_factors] host array + PathSet.move(1)
            ms per round including the final synchronisation, and whether the two labellings are equal.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--labels", type=int, default=32)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--speculation", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--skip-labels", action="store_true")
    a = ap.parse_args()
    import torch
    from lp_mp_amd import build as B, engine as E, model as M, synthetic as S
    import bench
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the engine has no CPU path")
    G, L = a.grid, a.labels
    e = E.Engine(0)
    stream_ptr = torch.cuda.current_stream().cuda_stream      # as bench.py: the engine works on torch's stream
    m, const, dual = bench.build_device_grid(torch, G, G, L, "dense", "colour_major", a.seed, E, S, stream_ptr)
    e.set_stream(stream_ptr)
    e.upload(m, const_dev=const.data_ptr(), dual_dev=dual.data_ptr(), keep=(const, dual))
    e.set_reparametrization(M.REPAM_ANISOTROPIC)
    have_dev = hasattr(e.L, "lpmp_lower_bound_dev")
    out = dict(tool="primal_state_probe", grid=G, labels=L, iters=a.iters, n_factors=int(m.n_factors),
               library="this tree's" if E.library_path() == B.SO else os.path.basename(E.library_path()),
               library_source_hash=B.source_hash() if E.library_path() == B.SO else None, has_device_calls=have_dev, scalars={})
    cell = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def loop(kind, n):
        last = None
        for _ in range(n):
            e.compute_pass(1)
            if kind == "host":
                last = e.lower_bound()
            else:
                e.lower_bound(cell.data_ptr())
        e.synchronize()
        return last if kind == "host" else float(cell.cpu()[0])

    variants = [(k, s) for s in (0, a.speculation) for k in (("host", "dev") if have_dev else ("host",))]
    for k, s in variants:
        out["scalars"]["%s_spec%d" % (k, s)] = dict(ms_per_iteration=[], last_bound_hex=None)
    for rep in range(a.repeat + 1):                       # (repetition 0 is the warm-up: schedules, joined launches, tracked bounds)
        for k, s in variants:
            e.set_speculation(s)
            loop(k, a.warmup)
            t0 = time.perf_counter()
            last = loop(k, a.iters)
            ms = (time.perf_counter() - t0) * 1e3 / a.iters
            if rep:
                row = out["scalars"]["%s_spec%d" % (k, s)]
                row["ms_per_iteration"].append(ms)
                row["last_bound_hex"] = struct.pack(">d", last).hex()
    out["speculation_stats"] = e.speculation_stats()
    e.set_speculation(0)
    # the bound alone, on tracked bounds with nothing stale: the cost of one call with and without the round trip
    alone = {}
    for k in ("host", "dev") if have_dev else ("host",):
        e.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            e.lower_bound() if k == "host" else e.lower_bound(cell.data_ptr())
        e.synchronize()
        alone[k] = (time.perf_counter() - t0) * 1e3 / 200
    out["bound_alone_ms"] = alone
    if have_dev:
        e.lower_bound(cell.data_ptr())
        e.synchronize()
        out["bound_bits_equal"] = struct.pack(">d", float(cell.cpu()[0])) == struct.pack(">d", e.lower_bound())

    if have_dev and not a.skip_labels:
        u = np.flatnonzero(m.f_kind == M.F_VECTOR).astype(np.int32)
        lab = np.random.default_rng(a.seed).integers(0, L, len(u)).astype(np.int32)
        primal = np.zeros((m.n_factors, 2), np.int32)
        primal[u, 0] = lab
        side = np.array([t.param for t in m.mtypes], np.int64)[m.m_type]
        primal[m.m_right, side] = primal[m.m_left, 0]
        lab_dev = torch.from_numpy(lab).cuda()
        torch.cuda.synchronize()
        groups = S.grid_paths(G, G, "colour_major")
        ps, r = e.path_set(groups), e.readout()
        res = {"set_labels": [], "upload_primal": []}
        got = {}
        for rep in range(a.repeat + 1):
            for k in ("set_labels", "upload_primal"):
                e.synchronize()
                t0 = time.perf_counter()
                if k == "set_labels":
                    r.set_labels(src_dev=lab_dev.data_ptr())
                else:
                    e.upload_primal(primal)
                ps.move(1)
                e.synchronize()
                if rep:
                    res[k].append((time.perf_counter() - t0) * 1e3)
                got[k] = r.labels()
        out["label_rounds"] = dict(ms_per_round=res, labels_equal=bool(np.array_equal(got["set_labels"], got["upload_primal"])),
                             n_paths=int(ps.n_paths), primal_cost_hex=struct.pack(">d", e.evaluate_primal()).hex())
        ps.close(); r.close()
    e.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
