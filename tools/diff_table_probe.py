#!/usr/bin/env python3
"""Times compute_pass on a grid of difference-indexed pairwise factors (LPMP_F_PAIRWISE_DIFF) and, with --expansion, on its
dense expansion on the same engine build.  GPU only: there is no CPU path, a missing device is an error.

    python tools/diff_table_probe.py --grid 512 --labels 128 --tables 2 --potential linear --warmup 5 --steps 20 --expansion --repeat 5
    python tools/diff_table_probe.py --grid 512 --labels 128 --trunc-labels 2 --warmup 5 --steps 20 --repeat 5
    python tools/diff_table_probe.py --capacity-check --grid 1024 --labels 128

Comparison mode: --repeat repetitions ALTERNATE the DIFF model and the expansion (two engines held side by side, warm-up and
timed passes in every repetition); the expansion's tables, 8 L^2 bytes per edge, are built in device memory from the same
vectors and scales with one multiply per entry (what expand_diff() does on the host), and after the last repetition the duals
of the two engines are compared.  --shared also times the same potentials as SHARED factors (<= 32 labels).
--trunc-labels K truncates the potentials after K label steps instead of LABELS / 4 (the band of the vectors, and which launches
run the banded kernel, are printed: bands, diff_band_info); duals_sha256 lets two libraries (LPMP_ENGINE_SO) be compared bit for bit.
Capacity-check mode: a DIFF grid that has no dense counterpart that fits; 5 + 20 single passes, the bound after every pass
must be finite and non-decreasing, and the tracked bound must agree with a recomputation of every factor to 1e-9 relative.
Prints one JSON line."""
from __future__ import annotations

import argparse
import dataclasses
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def vectors(potential: str, L: int, T: int, seed: int, trunc_labels: int = 0):
    """``trunc_labels`` K: the potential is truncated after K label steps (constant from |a - b| = K on; 0: after L / 4)"""
    from lp_mp_amd import model as M, synthetic as S
    K = trunc_labels if trunc_labels > 0 else L // 4
    if potential == "linear":
        return np.stack([M.truncated_linear(L, L, 0.02 * (t + 1), 0.02 * (t + 1) * K) for t in range(T)])
    if potential == "quadratic":
        return np.stack([M.truncated_quadratic(L, L, 0.002 * (t + 1), 0.002 * (t + 1) * K ** 2) for t in range(T)])
    return S.u01(T * (2 * L - 1), seed + 1000).reshape(T, 2 * L - 1)


def device_expansion(m):
    """(dense model without host constants, torch tensor of its tables on the device)"""
    import torch
    from lp_mp_amd import model as M
    df = np.nonzero(m.f_kind == M.F_PAIRWISE_DIFF)[0]
    assert df.shape[0] and np.all(np.diff(df) == 1) and int(m.const_sizes()[:df[0]].sum()) == 0, "the probe's grids: unaries, then the DIFF factors"
    L = int(m.f_dim0[df[0]])
    E = df.shape[0]
    vec = torch.from_numpy(np.ascontiguousarray(m.sh_data.reshape(m.n_shared_tables, 2 * L - 1))).cuda()
    ids = torch.from_numpy(m.f_table[df].astype(np.int64)).cuda()
    scale = torch.from_numpy(np.ascontiguousarray(m.const_data[:E])).cuda()
    idx = (torch.arange(L)[:, None] - torch.arange(L)[None, :] + (L - 1)).cuda()
    out = torch.empty((E, L, L), dtype=torch.float64, device="cuda")
    step = max(1, (1 << 26) // (L * L))
    for b in range(0, E, step):
        out[b:b + step] = scale[b:b + step, None, None] * vec[ids[b:b + step]][:, idx]
    torch.cuda.synchronize()
    kind = m.f_kind.copy()
    kind[df] = M.F_PAIRWISE_DENSE
    x = dataclasses.replace(m, f_kind=kind, const_data=None, sh_off=None, sh_dim0=None, sh_dim1=None, sh_data=None, f_table=None, _keep=[])
    return x, out


def timed(e, warmup: int, steps: int) -> float:
    e.compute_pass(max(1, warmup))
    e.synchronize()
    t0 = time.perf_counter()
    e.compute_pass(steps)
    e.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def kernel_times(e, steps: int) -> dict:
    e.enable_kernel_timing(True)
    e.reset_kernel_timing()
    e.compute_pass(steps)
    e.synchronize()
    t = e.kernel_timing()
    e.enable_kernel_timing(False)
    return {k: dict(v, ms_per_pass=v["ms"] / steps) for k, v in t.items()}


def comparison(a, out) -> int:
    import torch
    from lp_mp_amd import build as B, model as M, synthetic as S
    from lp_mp_amd.engine import Engine
    mode = M.REPAM_NAMES[a.mode]
    vec = vectors(a.potential, a.labels, a.tables, a.seed, a.trunc_labels)
    m = S.grid_model(a.grid, a.grid, a.labels, pairwise="diff", order=a.order, seed=a.seed, diff_tables=vec)
    from lp_mp_amd import engine as EG
    out.update(dual_bytes=int(m.dual_data.nbytes), library_source_hash=B.source_hash(), library=EG.library_path(),
               bands=[list(M.diff_band(v)) + [bool(M.diff_band_is_banded(v))] for v in vec])
    e = Engine(0)
    e.upload(m)
    e.set_reparametrization(mode)
    e.prepare_passes(a.steps)
    if hasattr(e.L, "lpmp_plan_diff_band_info"):     # (absent in an older library loaded through LPMP_ENGINE_SO for an A/B)
        out["diff_band_info"] = [e.plan.diff_band_info(d, mode) for d in (0, 1)]
    info = e.plan.pass_schedule_info(mode)
    out["diff"] = dict(classes_forward=e.plan.schedule_classes(0, mode), classes_backward=e.plan.schedule_classes(1, mode),
                       algorithmic_bytes_per_pass=int(info["algorithmic_bytes"]), n_launches_per_pass=int(info["n_launches"]), ms_per_pass=[])
    x_eng = None
    if a.expansion:
        x, tables = device_expansion(m)
        out["expanded_const_bytes"] = int(tables.numel() * 8)
        x_eng = Engine(0)
        x_eng.upload(x, const_dev=tables.data_ptr(), keep=tables)
        x_eng.set_reparametrization(mode)
        x_eng.prepare_passes(a.steps)
        xi = x_eng.plan.pass_schedule_info(mode)
        out["expansion"] = dict(classes_forward=x_eng.plan.schedule_classes(0, mode), algorithmic_bytes_per_pass=int(xi["algorithmic_bytes"]), ms_per_pass=[])
    for _ in range(a.repeat):
        out["diff"]["ms_per_pass"].append(timed(e, a.warmup, a.steps))
        if x_eng is not None:
            out["expansion"]["ms_per_pass"].append(timed(x_eng, a.warmup, a.steps))
    out["diff"]["lower_bound"] = e.lower_bound()
    out["diff"]["duals_sha256"] = hashlib.sha256(e.download_duals().tobytes()).hexdigest()   # (two libraries: equal digests = equal bits)
    if x_eng is not None:
        out["expansion"]["lower_bound"] = x_eng.lower_bound()
        out["duals_equal"] = bool(np.array_equal(e.download_duals(), x_eng.download_duals()))
        out["ratio_expansion_over_diff"] = [y / z for y, z in zip(out["expansion"]["ms_per_pass"], out["diff"]["ms_per_pass"])]
        out["diff_faster_in_every_repetition"] = all(r > 1.0 for r in out["ratio_expansion_over_diff"])
        out["expansion"]["kernel_timing"] = kernel_times(x_eng, a.steps)
        x_eng.close()
        del tables
    out["diff"]["kernel_timing"] = kernel_times(e, a.steps)
    out["device_memory_used_bytes"] = int(torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0])
    e.close()
    if a.shared:
        idx = np.arange(a.labels)[:, None] - np.arange(a.labels)[None, :] + (a.labels - 1)
        s = S.grid_model(a.grid, a.grid, a.labels, pairwise="shared", order=a.order, seed=a.seed, shared_tables=vec[:, idx], scales=m.const_data)
        e = Engine(0)
        e.upload(s); e.set_reparametrization(mode); e.prepare_passes(a.steps)
        out["shared"] = dict(classes_forward=e.plan.schedule_classes(0, mode), ms_per_pass=[timed(e, a.warmup, a.steps) for _ in range(a.repeat)])
        e.close()
    return 0


def capacity(a, out) -> int:
    import torch
    from lp_mp_amd import build as B, model as M, synthetic as S
    from lp_mp_amd.engine import Engine
    mode = M.REPAM_NAMES[a.mode]
    m = S.grid_model(a.grid, a.grid, a.labels, pairwise="diff", order=a.order, seed=a.seed, diff_tables=vectors(a.potential, a.labels, a.tables, a.seed, a.trunc_labels))
    edges = int((m.f_kind == M.F_PAIRWISE_DIFF).sum())
    out.update(dual_bytes=int(m.dual_data.nbytes), dense_counterpart_bytes=edges * 8 * a.labels * a.labels, library_source_hash=B.source_hash())
    e = Engine(0)
    e.upload(m)
    e.set_reparametrization(mode)
    out["classes_forward"] = e.plan.schedule_classes(0, mode)
    lbs = [e.lower_bound()]
    t = 0.0
    for i in range(a.warmup + a.steps):
        e.synchronize()
        t0 = time.perf_counter()
        e.compute_pass(1)
        e.synchronize()
        if i >= a.warmup:
            t += time.perf_counter() - t0
        lbs.append(e.lower_bound())
    tracked = lbs[-1]
    n_tracked = m.n_factors - e.lower_bound_recomputed()
    e.invalidate_lower_bounds()
    full = e.lower_bound()
    ok_mono = all(np.isfinite(x) for x in lbs) and all(y >= x - 1e-9 * max(1.0, abs(x)) for x, y in zip(lbs, lbs[1:]))
    ok_lb = abs(tracked - full) <= 1e-9 * max(1.0, abs(full)) and e.lower_bound_recomputed() == m.n_factors
    out.update(ms_per_pass=t * 1e3 / a.steps, lower_bounds=lbs, tracked_bound=tracked, recomputed_bound=full, factors_tracked_by_the_sweep=int(n_tracked),
               bounds_finite_and_non_decreasing=bool(ok_mono), tracked_equals_recomputed=bool(ok_lb),
               device_memory_used_bytes=int(torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]))
    e.close()
    return 0 if ok_mono and ok_lb else 1


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=512, help="the grid is GRID x GRID")
    ap.add_argument("--labels", type=int, default=128)
    ap.add_argument("--tables", type=int, default=2)
    ap.add_argument("--potential", default="linear", choices=["linear", "quadratic", "random"])
    ap.add_argument("--trunc-labels", type=int, default=0, help="truncate the potential after K label steps instead of LABELS / 4")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=1, help="repetitions, alternating DIFF and expansion")
    ap.add_argument("--order", default="colour_major", choices=["colour_major", "row_major"])
    ap.add_argument("--mode", default="anisotropic", choices=["anisotropic", "anisotropic2", "uniform", "damped_uniform"])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--expansion", action="store_true", help="also time the dense expansion (built in device memory)")
    ap.add_argument("--shared", action="store_true", help="also time the same potentials as SHARED factors (at most 32 labels for its fast class)")
    ap.add_argument("--capacity-check", action="store_true", help="capacity mode: bounds finite and non-decreasing, tracked bound = recomputed bound")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("diff_table_probe: no GPU", file=sys.stderr)
        return 2
    out = dict(mode_of_run="capacity-check" if a.capacity_check else "comparison", grid=a.grid, labels=a.labels, tables=a.tables,
               potential=a.potential, trunc_labels=a.trunc_labels, order=a.order, mode=a.mode, warmup=a.warmup, steps=a.steps, repeat=a.repeat, device=torch.cuda.get_device_name(0))
    rc = capacity(a, out) if a.capacity_check else comparison(a, out)
    print(json.dumps(out))
    return rc


if __name__ == "__main__":
    sys.exit(main())
