#!/usr/bin/env python3
"""Times the prepared read-outs (lpmp_readout_*) on the headline grid against what the library offered before.  GPU
only: there is no CPU path.

    python tools/readout_probe.py --grid 1024 --labels 32
    python tools/readout_probe.py --grid 1024 --labels 32 --pairwise shared

One engine runs 5 anisotropic passes (colour-major order) and a decode, then a read-out of every unary is created and timed:

    labels   into a device array            against  lpmp_download_primal (2 * n_factors int32 to the host)
    vectors  into a device array            against  lpmp_download_duals (the whole packed dual array to the host)
    beliefs  into a device array            against  one lpmp_compute_forward_pass (it reads the same deg * L^2 table entries)

Every figure is wall-clock time of the call between two synchronisations of the engine's stream, in ms: the FIRST call of the
read-out on its own (for the beliefs it builds and uploads the link tables), then one more warm-up call that is dropped, then
--repeat timed calls of which median, min and max are reported (the calls themselves, `ms`, too).  Prints one JSON line with the
library's source hash; --out writes it to a file."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(ms):
    s = sorted(ms)
    return dict(median_ms=s[len(s) // 2], min_ms=s[0], max_ms=s[-1], ms=ms)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=1024, help="the grid is GRID x GRID")
    ap.add_argument("--labels", type=int, default=32)
    ap.add_argument("--pairwise", default="dense", choices=["dense", "shared"])
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("readout_probe: no GPU", file=sys.stderr)
        return 2
    import numpy as np
    from lp_mp_amd import build as B, engine as E, model as M, synthetic as S
    H = W = a.grid
    L = a.labels
    sp = torch.cuda.current_stream().cuda_stream
    keep, kw = (), {}
    if a.pairwise == "dense":       # structure on the host, tables generated in HBM as bench.py generates them
        n, n_e = H * W, len(S.grid_edges(H, W)[0])
        m = S.grid_model(H, W, L, order="colour_major", seed=a.seed, device_const=True)
        const = torch.empty(n_e * L * L, dtype=torch.float64, device="cuda:0")
        E.synth_fill(const.data_ptr(), const.numel(), a.seed, n * L, sp)
        torch.cuda.synchronize()
        keep, kw = (const,), dict(const_dev=const.data_ptr())
    else:
        m = S.grid_model(H, W, L, pairwise="shared", order="colour_major", seed=a.seed)
    out = dict(grid=a.grid, labels=L, pairwise=a.pairwise, order="colour_major", repeat=a.repeat, passes="5 anisotropic",
               library_source_hash=B.source_hash(), device=torch.cuda.get_device_name(0))
    e = E.Engine(0)
    e.set_stream(sp)
    e.upload(m, keep=keep, **kw)
    e.set_reparametrization(M.REPAM_ANISOTROPIC)
    e.compute_pass(5)
    e.decode_primal(0, 0)
    e.synchronize()

    def wall(f):
        e.synchronize()
        t0 = time.perf_counter()
        f()
        e.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def series(f, repeat=a.repeat):
        first = wall(f)
        wall(f)                                   # warm-up, dropped
        return dict(stats([wall(f) for _ in range(repeat)]), first_call_ms=first)

    n_u = int((m.f_kind == M.F_VECTOR).sum())
    t0 = time.perf_counter()
    r = e.readout()
    out["create_ms"] = (time.perf_counter() - t0) * 1e3
    out["rows"], out["max_labels"] = r.n, r.max_labels
    assert r.n == n_u and r.max_labels == L
    lab = torch.empty(n_u, dtype=torch.int32, device="cuda:0")
    rows = torch.empty(n_u * L, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    built = e.schedules_built()
    out["labels_device"] = series(lambda: r.labels(lab.data_ptr()))
    out["download_primal"] = series(lambda: e.download_primal())
    out["vectors_device"] = series(lambda: r.vectors(rows.data_ptr(), L))
    out["download_duals"] = series(lambda: e.download_duals(), repeat=3)
    out["dual_bytes"] = int(m.dual_sizes().sum()) * 8
    out["beliefs_device"] = series(lambda: r.beliefs(rows.data_ptr(), L))
    out["schedules_built_by_the_readout"] = e.schedules_built() - built
    # which side costs what: in the colour-major order every unary of the first colour is on side 0 of all its pairwise factors and
    # every unary of the second colour on side 1 (variable i < j: i is the row index), so two half read-outs separate the two loops
    us = np.flatnonzero(m.f_kind == M.F_VECTOR)
    side = np.array([t.param for t in m.mtypes], np.int64)[m.m_type]
    sides_of = [np.unique(side[np.isin(m.m_left, part)]).tolist() for part in (us[:(n_u + 1) // 2], us[(n_u + 1) // 2:])]
    out["sides_of_the_halves"] = sides_of
    if sides_of == [[0], [1]]:
        for s, part in ((0, us[:(n_u + 1) // 2]), (1, us[(n_u + 1) // 2:])):
            rh = e.readout(part)
            out["beliefs_side%d_half" % s] = series(lambda: rh.beliefs(rows.data_ptr(), L))
            rh.close()
    out["forward_pass"] = series(lambda: e.forward_pass())
    # what was read out is what the old calls give: labels against download_primal, a few belief rows finite
    pr = e.download_primal()
    r.labels(lab.data_ptr()); e.synchronize()
    out["labels_equal_download_primal"] = bool(np.array_equal(lab.cpu().numpy(), pr[us, 0]))
    out["beliefs_over_forward_pass"] = out["beliefs_device"]["median_ms"] / out["forward_pass"]["median_ms"]
    out["labels_over_download_primal"] = out["labels_device"]["median_ms"] / out["download_primal"]["median_ms"]
    out["vectors_over_download_duals"] = out["vectors_device"]["median_ms"] / out["download_duals"]["median_ms"]
    r.close()
    e.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if out["labels_equal_download_primal"] else 1


if __name__ == "__main__":
    sys.exit(main())
