#!/usr/bin/env python3
"""Times lpmp_decode_primal (labels from the duals by conditional rounding) on the headline grid against the
rounding pass.  GPU only: there is no CPU path.

    python tools/decode_probe.py --grid 1024 --labels 32
    python tools/decode_probe.py --grid 1024 --labels 128 --pairwise diff

Engine A runs 5 + 20 anisotropic passes (colour-major order) and then, for refine in {0, 2}, one warm-up decode and --repeat
timed ones (HIP events on the engine's stream around the call): median, min, max and the energy (`evaluate_primal`).  Engine B runs
the same passes — the same duals, checked through the lower bound — and then the facility the library had before:
`compute_pass_and_primal` under `damped_uniform` + `evaluate_primal`, timed the same way (every repetition is a further pass).
One plain anisotropic pass of A is timed for scale.  Prints one JSON line with the library's source hash; --out writes it to a file."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(ms):
    s = sorted(ms)
    return dict(median_ms=s[len(s) // 2], min_ms=s[0], max_ms=s[-1], ms=ms)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=1024, help="the grid is GRID x GRID")
    ap.add_argument("--labels", type=int, default=32)
    ap.add_argument("--pairwise", default="dense", choices=["dense", "diff"])
    ap.add_argument("--order", default="colour_major", choices=["colour_major", "row_major"])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("decode_probe: no GPU", file=sys.stderr)
        return 2
    from lp_mp_amd import build as B, engine as E, model as M, synthetic as S
    H = W = a.grid
    L = a.labels
    sp = torch.cuda.current_stream().cuda_stream
    keep, kw = (), {}
    if a.pairwise == "dense":       # structure on the host, tables generated in HBM as bench.py generates them
        n, n_e = H * W, len(S.grid_edges(H, W)[0])
        m = S.grid_model(H, W, L, order=a.order, seed=a.seed, device_const=True, compute_primal=True)
        const = torch.empty(n_e * L * L, dtype=torch.float64, device="cuda:0")
        E.synth_fill(const.data_ptr(), const.numel(), a.seed, n * L, sp)
        torch.cuda.synchronize()
        keep, kw = (const,), dict(const_dev=const.data_ptr())
    else:                           # truncated linear after 2 label steps, two vectors, random scales
        import numpy as np
        D = np.stack([M.truncated_linear(L, L, 0.05, 0.1), M.truncated_linear(L, L, 0.02, 0.04)])
        m = S.grid_model(H, W, L, pairwise="diff", order=a.order, seed=a.seed, diff_tables=D, compute_primal=True)
    out = dict(grid=a.grid, labels=L, pairwise=a.pairwise, order=a.order, repeat=a.repeat, passes="5 + 20 anisotropic",
               library_source_hash=B.source_hash(), device=torch.cuda.get_device_name(0))

    def engine():
        e = E.Engine(0)
        e.set_stream(sp)
        e.upload(m, keep=keep, **kw)
        e.set_reparametrization(M.REPAM_ANISOTROPIC)
        e.compute_pass(5); e.compute_pass(20)
        return e

    def timed(f, n):
        ms = []
        for i in range(n):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); f(i); t1.record(); t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return ms

    ea = engine()
    out["lower_bound"] = ea.lower_bound()
    out["decode_structure"] = ea.plan.decode_info(0)
    for refine in (0, 2):
        ea.decode_primal(0, refine)                       # warm-up (the first one also builds the device tables)
        r = stats(timed(lambda i: ea.decode_primal(0, refine), a.repeat))
        r["energy"] = ea.evaluate_primal()
        r["consistent"] = ea.check_primal_consistency()
        out["decode_refine%d" % refine] = r
    out["lower_bound_after_decodes"] = ea.lower_bound()
    out["plain_pass"] = stats(timed(lambda i: ea.compute_pass(1), a.repeat + 1)[1:])
    ea.close()
    eb = engine()
    out["second_engine_same_bound"] = eb.lower_bound() == out["lower_bound"]
    eb.set_reparametrization(M.REPAM_DAMPED_UNIFORM)
    eb.compute_pass_and_primal(1)                         # warm-up (builds the damped_uniform schedules)
    energies = []

    def rounding(i):
        eb.compute_pass_and_primal(i + 2)
    ms = []
    for i in range(a.repeat):
        ms += timed(lambda _: rounding(i), 1)
        energies.append(eb.evaluate_primal())
    out["rounding_pass"] = dict(stats(ms), energies=energies, energy_first=None)
    ev = timed(lambda i: eb.evaluate_primal(), a.repeat)
    out["evaluate_primal"] = stats(ev)
    eb.close()
    # the rounding energy on the SAME duals as the decode: a third engine, one rounding pass right after the 25 passes
    ec = engine()
    ec.set_reparametrization(M.REPAM_DAMPED_UNIFORM)
    ec.compute_pass_and_primal(1)
    out["rounding_pass"]["energy_first"] = ec.evaluate_primal()
    ec.close()
    out["decode_over_plain_pass"] = out["decode_refine0"]["median_ms"] / out["plain_pass"]["median_ms"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if out["lower_bound_after_decodes"] == out["lower_bound"] and out["decode_refine0"]["consistent"] else 1


if __name__ == "__main__":
    sys.exit(main())
