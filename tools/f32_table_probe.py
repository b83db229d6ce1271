#!/usr/bin/env python3
"""Times compute_pass on a dense grid with the tables stored as doubles (engine A) and as floats (engine B, strict mode) — the
SAME float-valued tables, generated in HBM as bench.py generates C3's and rounded there.  GPU only: there is no CPU path.

    python tools/f32_table_probe.py --grid 1024 --labels 32 --warmup 5 --steps 20 --repeat 5

A repetition runs warm-up + steps passes (joined calls) on A, then on B; both engines therefore execute the same passes, and after
all of them their dual buffers must be bit-identical: the correctness check at a size no CPU oracle reaches.  Prints one JSON
line: ms per pass of every repetition for each engine (host clock around a synchronise), their ratio, the algorithmic bytes of a
pass under each accounting, device memory, and the per-class kernel timing of a separate, event-timed run.

--f32-only: engine B alone (sizes whose f64 engine is not wanted).  Checked instead: the lower bound after every repetition is
finite and does not decrease, and the tracked bound equals the recomputed one within 1e-9 relative.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def device_grid(torch, E, S, H, W, L, order, seed):
    """structure on the host, unaries and tables generated in HBM; the tables rounded to float values in place, piece by piece"""
    dev = torch.device("cuda", torch.cuda.current_device())
    n, n_e = H * W, len(S.grid_edges(H, W)[0])
    m = S.grid_model(H, W, L, order=order, seed=seed, device_const=True)
    const = torch.empty(n_e * L * L, dtype=torch.float64, device=dev)
    dual = torch.zeros(n * L + n_e * 2 * L, dtype=torch.float64, device=dev)
    sp = torch.cuda.current_stream().cuda_stream
    E.synth_fill(const.data_ptr(), const.numel(), seed, n * L, sp)
    E.synth_fill(dual.data_ptr(), n * L, seed, 0, sp)
    step = 1 << 26
    for i in range(0, const.numel(), step):
        const[i:i + step] = const[i:i + step].float().double()
    torch.cuda.synchronize()
    return m, const, dual


def timed(torch, e, warmup, steps):
    e.compute_pass(max(1, warmup))
    e.synchronize()
    t0 = time.perf_counter()
    e.compute_pass(steps)
    e.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=1024, help="the grid is GRID x GRID")
    ap.add_argument("--labels", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--order", default="colour_major", choices=["colour_major", "row_major"])
    ap.add_argument("--mode", default="anisotropic", choices=["anisotropic", "anisotropic2", "uniform", "damped_uniform"])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--f32-only", action="store_true")
    ap.add_argument("--no-kernel-timing", action="store_true", help="skip the event-timed run (a profiler run collects its own)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("f32_table_probe: no GPU", file=sys.stderr)
        return 2
    from lp_mp_amd import engine as E, model as M, synthetic as S
    mode = M.REPAM_NAMES[a.mode]
    m, const, dual_b = device_grid(torch, E, S, a.grid, a.grid, a.labels, a.order, a.seed)
    out = dict(grid=a.grid, labels=a.labels, order=a.order, mode=a.mode, warmup=a.warmup, steps=a.steps, repeat=a.repeat,
               f64_table_bytes=int(const.numel() * 8), dual_bytes=int(dual_b.numel() * 8), device=torch.cuda.get_device_name(0))
    engines = []
    if not a.f32_only:
        dual_a = dual_b.clone()
        engines.append(("f64", dual_a))
    engines.append(("f32", dual_b))
    run = {}
    for prec, dual in engines:
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        e = E.Engine(0)
        e.upload(m, const_dev=const.data_ptr(), dual_dev=dual.data_ptr(), keep=(const, dual), rows_layout=False, table_precision=prec)
        e.set_reparametrization(mode)
        e.prepare_passes(a.warmup); e.prepare_passes(a.steps)
        e.synchronize()
        info = e.plan.pass_schedule_info(mode)
        run[prec] = dict(engine=e, ms=[], lower_bounds=[e.lower_bound()])
        out[prec] = dict(table_precision=e.table_precision(), engine_device_bytes=int(free0 - torch.cuda.mem_get_info()[0]),
                         algorithmic_bytes_per_pass=int(info["algorithmic_bytes"]), classes_forward=e.plan.schedule_classes(0, mode))
    for _ in range(a.repeat):                       # the engines alternate
        for prec, _d in engines:
            r = run[prec]
            r["ms"].append(timed(torch, r["engine"], a.warmup, a.steps))
            r["lower_bounds"].append(r["engine"].lower_bound())
    for prec, _d in engines:
        r = run[prec]
        out[prec]["ms_per_pass"] = r["ms"]
        out[prec]["lower_bounds"] = r["lower_bounds"]
        med = sorted(r["ms"])[len(r["ms"]) // 2]
        out[prec]["median_ms_per_pass"] = med
        out[prec]["algorithmic_gb_per_s"] = out[prec]["algorithmic_bytes_per_pass"] / med / 1e6
    ok = True
    if a.f32_only:
        import math
        lbs = run["f32"]["lower_bounds"]
        e = run["f32"]["engine"]
        tracked = e.lower_bound()
        e.invalidate_lower_bounds()
        recomputed = e.lower_bound()
        out["f32"]["tracked_bound"], out["f32"]["recomputed_bound"] = tracked, recomputed
        out["bounds_finite_and_non_decreasing"] = all(math.isfinite(x) for x in lbs) and all(y >= x - 1e-9 * max(1.0, abs(x)) for x, y in zip(lbs, lbs[1:]))
        out["tracked_equals_recomputed"] = abs(tracked - recomputed) <= 1e-9 * max(1.0, abs(recomputed))
        ok = out["bounds_finite_and_non_decreasing"] and out["tracked_equals_recomputed"]
    else:
        for prec, _d in engines:
            run[prec]["engine"].synchronize()
        torch.cuda.synchronize()
        out["duals_bit_identical"] = bool(torch.equal(engines[0][1], engines[1][1]))
        out["ratio_f32_over_f64"] = [b / x for x, b in zip(run["f64"]["ms"], run["f32"]["ms"])]
        out["f32_faster_in_every_repetition"] = all(r < 1.0 for r in out["ratio_f32_over_f64"])
        ok = out["duals_bit_identical"]
    out["device_bytes_in_use"] = int(torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0])
    if not a.no_kernel_timing:
        for prec, _d in engines:                    # event-timed launches, one launch per step: a run of its own, after the checks
            e = run[prec]["engine"]
            e.enable_kernel_timing(True); e.reset_kernel_timing()
            e.compute_pass(a.steps); e.synchronize()
            out[prec]["kernel_timing"] = {k: dict(v, ms_per_pass=v["ms"] / a.steps) for k, v in e.kernel_timing().items()}
            e.enable_kernel_timing(False)
    for prec, _d in engines:
        run[prec]["engine"].close()
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
