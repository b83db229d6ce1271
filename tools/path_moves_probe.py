#!/usr/bin/env python3
"""Times lpmp_path_moves (exact relabelling of rows and columns given all other labels) on a grid against the decode,
its refinement sweeps and a sweep of the same build.  GPU only: there is no CPU path.

    python tools/path_moves_probe.py --rows 1024 --cols 1024 --labels 32 --passes 5,50
    python tools/path_moves_probe.py --rows 512 --cols 512 --labels 128 --pairwise diff
    python tools/path_moves_probe.py --rows 256 --cols 4096 --labels 32        (few long paths in two of the four groups)

One engine in colour-major order, anisotropic passes.  After each pass count of --passes: the bound, and primal cost
(`evaluate_primal`) and milliseconds (HIP events on the engine's stream around the call; median, min, max of --repeat) of
  decode                 decode_primal(0, 0)
  decode + 3 sweeps      decode_primal(0, 3)
  + 1 / + 2 rounds       PathSet.move(1) / move(2) on the labels of a fresh decode_primal(0, 0) (the move alone is timed), and each
                         of the four groups of a round on its own
and a forward sweep and a whole pass for scale.  A second engine times the rounding pass (`compute_pass_and_primal` under
damped_uniform), the facility a round is held against.  Prints one JSON line with the library's source hash; --out writes it to a file."""
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
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--labels", type=int, default=32)
    ap.add_argument("--pairwise", default="dense", choices=["dense", "diff"])
    ap.add_argument("--passes", default="5,50", help="pass counts after which everything is measured, ascending")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-rounding", action="store_true", help="skip the second engine")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("path_moves_probe: no GPU", file=sys.stderr)
        return 2
    from lp_mp_amd import build as B, engine as E, model as M, synthetic as S
    H, W, L = a.rows, a.cols, a.labels
    sp = torch.cuda.current_stream().cuda_stream
    keep, kw = (), {}
    if a.pairwise == "dense":       # structure on the host, tables generated in HBM as bench.py generates them
        n, n_e = H * W, len(S.grid_edges(H, W)[0])
        m = S.grid_model(H, W, L, order="colour_major", seed=a.seed, device_const=True, compute_primal=True)
        const = torch.empty(n_e * L * L, dtype=torch.float64, device="cuda:0")
        E.synth_fill(const.data_ptr(), const.numel(), a.seed, n * L, sp)
        torch.cuda.synchronize()
        keep, kw = (const,), dict(const_dev=const.data_ptr())
    else:                           # truncated linear after 2 label steps, two vectors, random scales
        import numpy as np
        D = np.stack([M.truncated_linear(L, L, 0.05, 0.1), M.truncated_linear(L, L, 0.02, 0.04)])
        m = S.grid_model(H, W, L, pairwise="diff", order="colour_major", seed=a.seed, diff_tables=D, compute_primal=True)
    groups = S.grid_paths(H, W, "colour_major")
    out = dict(rows=H, cols=W, labels=L, pairwise=a.pairwise, order="colour_major", repeat=a.repeat, library_source_hash=B.source_hash(),
               device=torch.cuda.get_device_name(0), after_passes={})

    def engine():
        e = E.Engine(0)
        e.set_stream(sp)
        e.upload(m, keep=keep, **kw)
        e.set_reparametrization(M.REPAM_ANISOTROPIC)
        return e

    def timed(f, n, before=None):
        ms = []
        for i in range(n):
            if before:
                before()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); f(); t1.record(); t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return ms

    e = engine()
    ps = e.path_set(groups)
    singles = [e.path_set([g]) for g in groups]
    out["path_set"] = dict(n_groups=ps.n_groups, n_paths=ps.n_paths, longest=ps.longest, scratch_bytes=ps.scratch_bytes, structure=e.plan.path_info(groups))
    done, ok = 0, True
    for passes in [int(x) for x in a.passes.split(",")]:
        e.compute_pass(passes - done)
        done = passes
        r = dict(lower_bound=e.lower_bound())
        fresh = lambda: e.decode_primal(0, 0)
        for name, refine in (("decode", 0), ("decode_3_sweeps", 3)):
            e.decode_primal(0, refine)                    # warm-up (the first one also builds the device tables)
            r[name] = stats(timed(lambda: e.decode_primal(0, refine), a.repeat))
            r[name]["energy"] = e.evaluate_primal()
        prev = r["decode"]["energy"]
        for rounds in (1, 2):
            fresh(); ps.move(rounds)                      # warm-up
            s = stats(timed(lambda: ps.move(rounds), a.repeat, before=fresh))
            s["energy"] = e.evaluate_primal()
            s["consistent"] = e.check_primal_consistency()
            ok = ok and s["consistent"] and s["energy"] <= prev + 1e-9 * max(1.0, abs(prev))
            prev = s["energy"]
            r["rounds_%d" % rounds] = s
        for g in singles:
            g.move(1)                                     # warm-up
        fresh()
        r["groups_of_round_1_ms"] = [timed(lambda: g.move(1), 1)[0] for g in singles]
        r["lower_bound_after"] = e.lower_bound()
        ok = ok and r["lower_bound_after"] == r["lower_bound"]
        out["after_passes"][str(passes)] = r
    out["forward_sweep"] = stats(timed(lambda: e.forward_pass(), a.repeat + 1)[1:])
    e.backward_pass()
    out["plain_pass"] = stats(timed(lambda: e.compute_pass(1), a.repeat + 1)[1:])
    last = out["after_passes"][str(done)]
    out["round_over_plain_pass"] = last["rounds_1"]["median_ms"] / out["plain_pass"]["median_ms"]
    for s in singles:
        s.close()
    ps.close()
    e.close()
    if not a.no_rounding:
        eb = engine()
        eb.compute_pass(done)
        eb.set_reparametrization(M.REPAM_DAMPED_UNIFORM)
        eb.compute_pass_and_primal(1)                     # warm-up (builds the damped_uniform schedules)
        it = [1]

        def rounding():
            it[0] += 1
            eb.compute_pass_and_primal(it[0])
        out["rounding_pass"] = stats(timed(rounding, a.repeat))
        out["rounding_pass"]["energy_last"] = eb.evaluate_primal()
        out["round_over_rounding_pass"] = last["rounds_1"]["median_ms"] / out["rounding_pass"]["median_ms"]
        eb.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
