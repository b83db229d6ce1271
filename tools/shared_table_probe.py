#!/usr/bin/env python3
"""Times compute_pass on a grid whose pairwise factors share a handful of tables (LPMP_F_PAIRWISE_SHARED) and, with
--expand, on its expansion to one private dense table per edge.  GPU only: there is no CPU path, a missing device is an error.

    python tools/shared_table_probe.py --grid 1024 --labels 32 --tables 2 --warmup 5 --steps 20

Prints one JSON line: ms per pass (host clock around a synchronise, after a warm-up), the algorithmic bytes of a pass
(DESIGN.md accounting), the kernel classes of the sweep, and the per-class kernel timing of a separate, event-timed run.
--expand materialises the expansion with numpy on the host (8 L^2 bytes per edge): sizes whose expansion fits host memory only.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(model, warmup: int, steps: int, mode: int) -> dict:
    from lp_mp_amd.engine import Engine
    e = Engine(0)
    e.upload(model)
    e.set_reparametrization(mode)
    e.prepare_passes(steps)
    e.compute_pass(max(1, warmup))
    e.synchronize()
    t0 = time.perf_counter()
    e.compute_pass(steps)
    e.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    lb = e.lower_bound()
    info = e.plan.pass_schedule_info(mode)
    classes = [e.plan.schedule_classes(d, mode) for d in (0, 1)]
    # per-class kernel time: event-timed launches (one launch per step, no graph replay), in a run of its own
    e.enable_kernel_timing(True)
    e.reset_kernel_timing()
    e.compute_pass(steps)
    e.synchronize()
    timing = e.kernel_timing()
    e.enable_kernel_timing(False)
    e.close()
    out = dict(ms_per_pass=ms, lower_bound=lb, algorithmic_bytes_per_pass=int(info["algorithmic_bytes"]),
               n_launches_per_pass=int(info["n_launches"]), classes_forward=classes[0], classes_backward=classes[1],
               algorithmic_gb_per_s=info["algorithmic_bytes"] / ms / 1e6,
               kernel_timing={k: dict(v, ms_per_pass=v["ms"] / steps) for k, v in timing.items()})
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=1024, help="the grid is GRID x GRID")
    ap.add_argument("--labels", type=int, default=32)
    ap.add_argument("--tables", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--order", default="colour_major", choices=["colour_major", "row_major"])
    ap.add_argument("--mode", default="anisotropic", choices=["anisotropic", "anisotropic2", "uniform", "damped_uniform"])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--expand", action="store_true", help="also time the expansion (one private dense table per edge)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("shared_table_probe: no GPU", file=sys.stderr)
        return 2
    from lp_mp_amd import model as M, synthetic as S
    mode = M.REPAM_NAMES[a.mode]
    m = S.grid_model(a.grid, a.grid, a.labels, pairwise="shared", order=a.order, seed=a.seed, n_tables=a.tables)
    out = dict(grid=a.grid, labels=a.labels, tables=a.tables, order=a.order, mode=a.mode, warmup=a.warmup, steps=a.steps,
               dual_bytes=int(m.dual_data.nbytes), device=torch.cuda.get_device_name(0))
    out["shared"] = measure(m, a.warmup, a.steps, mode)
    if a.expand:
        x = m.expand_shared()
        out["expanded_const_bytes"] = int(x.const_data.nbytes)
        out["expanded"] = measure(x, a.warmup, a.steps, mode)
        out["speedup"] = out["expanded"]["ms_per_pass"] / out["shared"]["ms_per_pass"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
