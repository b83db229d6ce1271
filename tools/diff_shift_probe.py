#!/usr/bin/env python3
"""Times shifted difference-indexed pairwise factors (LPMP_F_PAIRWISE_DIFF_SHIFT).  GPU only: there is no CPU path, a missing
device is an error.

    python tools/diff_shift_probe.py --compare --grid 512 --labels 128 --warmup 5 --steps 20 --repeat 5
    python tools/diff_shift_probe.py --two-level --grid 256 --full-labels 256 --window 32 --passes 30 [--full]
    python tools/diff_shift_probe.py --windows --grid 512 --labels 128 --trunc-labels 2 --warmup 5 --steps 20 --repeat 1

--compare: a grid of DIFF_SHIFT factors with a random shift per edge against the plain DIFF grid of the same size, labels, vectors
(random ones: the plain grid runs the full kernel, not the banded one) and scales, two engines side by side, repetitions
alternating.  Also uploads the degenerate DIFF_SHIFT grid (n = 2L - 1, s = L - 1) once and compares its duals with the plain
grid's after the same passes (duals_equal_degenerate).
--two-level: a coarse DIFF model (FULL / STRIDE labels, every coarse label standing for STRIDE fine ones) -> decode_primal
-> a window of WINDOW labels per variable around its coarse estimate -> the DIFF_SHIFT model on the compact truncated-linear
vector -> decode_primal.  Reports the times and the energy of the final labelling evaluated on the full-range model (numpy, on
the host); --full also solves the full-range DIFF model for the same number of passes.
--windows: one level of a coarse-to-fine run on its own: a grid of DIFF_SHIFT factors over windows of LABELS labels around random
centres, on the compact truncated-linear vector of 2 TRUNC_LABELS + 1 entries (--trunc-labels K; or, with --band-width W, on a
vector whose band has W random entries between two unequal tails).  Such windows run sweep_diff_shift_band_kernel where the rule
admits the band ((W or 2 K - 1) * 4 <= 2 LABELS - 1) and sweep_diff_shift_kernel under LPMP_NO_DIFF_BAND=1 or with a library from
before the banded form (LPMP_ENGINE_SO): one process per run for an A/B.  Reports ms per pass, the kernels that ran and a digest
of the duals (two runs of one model: equal digests = equal bits).
Prints one JSON line."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def compare(a, out) -> int:
    from lp_mp_amd import build as B, model as M, synthetic as S
    from lp_mp_amd.engine import Engine
    mode = M.REPAM_NAMES[a.mode]
    G, L = a.grid, a.labels
    vec = S.u01(a.tables * (2 * L - 1), a.seed + 1000).reshape(a.tables, 2 * L - 1)
    plain = S.grid_model(G, G, L, pairwise="diff", order=a.order, seed=a.seed, diff_tables=vec)
    E = int((plain.f_kind == M.F_PAIRWISE_DIFF).sum())
    shifts = np.random.default_rng(a.seed).integers(0, 2 * L - 1, E)
    scales = plain.const_data[:E]
    shifted = S.grid_model(G, G, L, pairwise="diff_shift", order=a.order, seed=a.seed, diff_tables=vec, scales=scales, shifts=shifts)
    degenerate = S.grid_model(G, G, L, pairwise="diff_shift", order=a.order, seed=a.seed, diff_tables=vec, scales=scales)
    out.update(library_source_hash=B.source_hash(), dual_bytes=int(plain.dual_data.nbytes))
    eng = {}
    for name, m in (("diff", plain), ("diff_shift", shifted)):
        e = Engine(0)
        e.upload(m); e.set_reparametrization(mode); e.prepare_passes(a.steps)
        info = e.plan.pass_schedule_info(mode)
        out[name] = dict(classes_forward=e.plan.schedule_classes(0, mode), diff_band_info=e.plan.diff_band_info(0, mode),
                         algorithmic_bytes_per_pass=int(info["algorithmic_bytes"]), n_launches_per_pass=int(info["n_launches"]), ms_per_pass=[])
        eng[name] = e
    for _ in range(a.repeat):
        for name in ("diff", "diff_shift"):
            out[name]["ms_per_pass"].append(timed(eng[name], a.warmup, a.steps))
    for name in ("diff", "diff_shift"):
        out[name]["lower_bound"] = eng[name].lower_bound()
        out[name]["kernel_timing"] = kernel_times(eng[name], a.steps)
    out["ratio_shift_over_diff"] = [y / z for y, z in zip(out["diff_shift"]["ms_per_pass"], out["diff"]["ms_per_pass"])]
    out["diff"]["duals_sha256"] = hashlib.sha256(eng["diff"].download_duals().tobytes()).hexdigest()   # (two libraries: equal digests = equal bits)
    eng["diff_shift"].close()
    # the degenerate model against the plain one, from a fresh upload each: the same bits
    d = []
    for m in (plain, degenerate):
        eng["diff"].upload(m); eng["diff"].set_reparametrization(mode)
        eng["diff"].compute_pass(3)
        d.append(eng["diff"].download_duals())
    out["duals_equal_degenerate"] = bool(np.array_equal(d[0], d[1]))
    eng["diff"].close()
    return 0 if out["duals_equal_degenerate"] else 1


def windows(a, out) -> int:
    from lp_mp_amd import build as B, model as M, synthetic as S
    from lp_mp_amd.engine import Engine
    mode = M.REPAM_NAMES[a.mode]
    G, L = a.grid, a.labels
    n = G * G
    var = S.grid_variable_order(G, G, a.order).reshape(-1)
    ga, gb = S.grid_edges(G, G)
    ei, ej = np.minimum(var[ga], var[gb]), np.maximum(var[ga], var[gb])
    E = ei.shape[0]
    rng = np.random.default_rng(a.seed)
    if a.band_width is None:
        Dv, zero = M.truncated_linear_compact(a.slope, a.slope * a.trunc_labels)
    else:
        W = a.band_width
        Dv = np.concatenate([np.full(3, 2.0), rng.uniform(0.05, 1.0, W), np.full(3, 1.5)])
        zero = 3 + W // 2
    centres = rng.integers(0, max(1, a.centre_spread) + 1, n)      # neighbouring windows overlap: most bands lie inside the receive
    shifts = M.window_shift(centres[ei], centres[ej], zero)
    m = S.grid_model(G, G, L, pairwise="diff_shift", order=a.order, seed=a.seed, diff_tables=[Dv], shifts=shifts)
    lo, hi = M.diff_band(Dv)
    e = Engine(0)
    e.upload(m); e.set_reparametrization(mode); e.prepare_passes(a.steps)
    info = e.plan.pass_schedule_info(mode)
    out.update(labels=L, vector_entries=int(Dv.shape[0]), band=[lo, hi], band_width=hi - lo + 1, rule_admits=bool((hi - lo + 1) * M.DIFF_BAND_DIV <= 2 * L - 1),
               no_diff_band=os.environ.get("LPMP_NO_DIFF_BAND") is not None, library=os.environ.get("LPMP_ENGINE_SO", "tree"),
               library_source_hash=B.source_hash(), classes_forward=e.plan.schedule_classes(0, mode), n_launches_per_pass=int(info["n_launches"]),
               algorithmic_bytes_per_pass=int(info["algorithmic_bytes"]))
    if hasattr(e.L, "lpmp_plan_diff_shift_band_info"):      # (absent in a library from before the banded form)
        out["diff_shift_band_info"] = e.plan.diff_shift_band_info(0, mode)
    out["ms_per_pass"] = [timed(e, a.warmup, a.steps) for _ in range(a.repeat)]
    out["lower_bound"] = e.lower_bound()
    out["duals_sha256"] = hashlib.sha256(e.download_duals().tobytes()).hexdigest()
    out["kernel_timing"] = kernel_times(e, a.steps)
    e.close()
    return 0


def energy(un, ei, ej, scales, labels, slope, trunc) -> float:
    """the labelling on the full-range model: unaries + scale * min(slope * |x_i - x_j|, trunc), in numpy"""
    x = labels.astype(np.int64)
    pw = np.minimum(np.float64(slope) * np.abs(x[ei] - x[ej]).astype(np.float64), np.float64(trunc))
    return float(un[np.arange(un.shape[0]), x].sum() + (scales * pw).sum())


def two_level(a, out) -> int:
    from lp_mp_amd import model as M, synthetic as S
    from lp_mp_amd.engine import Engine
    mode = M.REPAM_NAMES[a.mode]
    G, F, Wn = a.grid, a.full_labels, a.window
    stride = a.stride
    Lc = F // stride
    n = G * G
    var = S.grid_variable_order(G, G, a.order).reshape(-1)
    ga, gb = S.grid_edges(G, G)
    ei, ej = np.minimum(var[ga], var[gb]), np.maximum(var[ga], var[gb])
    E = ei.shape[0]
    rng = np.random.default_rng(a.seed)
    # a smooth ground truth and noisy quadratic unaries around it: the coarse estimate means something
    yy, xx = np.divmod(np.arange(n), G)
    truth = np.empty(n)
    truth[var] = F / 2 + F / 3 * np.sin(yy / G * 5.0) * np.cos(xx / G * 4.0)     # (var: grid position -> variable)
    un = (np.arange(F)[None, :] - (truth + rng.normal(0, F / 16, n))[:, None]) ** 2 / (F * F / 16.0)
    scales = 0.5 + rng.uniform(0, 1, E)
    slope, trunc = a.slope, a.slope * a.trunc_labels
    t = {}

    def solve(name, m, passes):
        e = Engine(0)
        t0 = time.perf_counter()
        e.upload(m); e.set_reparametrization(mode); e.prepare_passes(passes)
        e.synchronize()
        t[name + "_upload_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        e.compute_pass(passes)
        e.synchronize()
        t[name + "_ms_per_pass"] = (time.perf_counter() - t0) * 1e3 / passes
        t0 = time.perf_counter()
        e.decode_primal(0, 1)
        lab = e.readout().labels()
        t[name + "_decode_ms"] = (time.perf_counter() - t0) * 1e3
        out[name] = dict(classes=e.plan.schedule_classes(0, mode), lower_bound=e.lower_bound(), dual_bytes=int(m.dual_data.nbytes))
        e.close()
        return lab.astype(np.int64)

    # coarse level: label k stands for the fine labels k * stride ... (k + 1) * stride - 1
    t0 = time.perf_counter()
    un_c = un.reshape(n, Lc, stride).min(axis=2)
    Dc_coarse = M.truncated_linear(Lc, Lc, slope * stride, trunc)
    coarse = S.mrf_model(n, Lc, ei, ej, un_c, compute_primal=True, diff=(Dc_coarse[None], np.zeros(E, np.int32), scales))
    t["coarse_build_s"] = time.perf_counter() - t0
    lab_c = solve("coarse", coarse, a.passes)
    # windows of Wn labels around the coarse estimate; the compact vector, one shift per edge
    t0 = time.perf_counter()
    c = np.clip(lab_c * stride + stride // 2 - Wn // 2, 0, F - Wn)
    Dv, zero = M.truncated_linear_compact(slope, trunc)
    un_w = np.take_along_axis(un, c[:, None] + np.arange(Wn)[None, :], axis=1)
    fine = S.mrf_model(n, Wn, ei, ej, un_w, compute_primal=True, diff_shift=([Dv], np.zeros(E, np.int32), scales, M.window_shift(c[ei], c[ej], zero)))
    t["window_build_s"] = time.perf_counter() - t0
    lab_w = solve("windowed", fine, a.passes)
    final = c + lab_w
    out.update(grid=G, full_labels=F, window=Wn, coarse_labels=Lc, compact_vector_entries=int(Dv.shape[0]),
               energy_coarse_estimate=energy(un, ei, ej, scales, np.clip(lab_c * stride + stride // 2, 0, F - 1), slope, trunc),
               energy_windowed=energy(un, ei, ej, scales, final, slope, trunc))
    if a.full:
        full = S.mrf_model(n, F, ei, ej, un, compute_primal=True, diff=(M.truncated_linear(F, F, slope, trunc)[None], np.zeros(E, np.int32), scales))
        out["energy_full_range"] = energy(un, ei, ej, scales, solve("full_range", full, a.passes), slope, trunc)
    out["times"] = t
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--two-level", action="store_true")
    ap.add_argument("--windows", action="store_true")
    ap.add_argument("--band-width", type=int, default=None, help="windows: a vector with a band of that many random entries instead of the truncated-linear one")
    ap.add_argument("--centre-spread", type=int, default=8, help="windows: the window centres are uniform in [0, SPREAD]")
    ap.add_argument("--grid", type=int, default=512, help="the grid is GRID x GRID")
    ap.add_argument("--labels", type=int, default=128)
    ap.add_argument("--tables", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--full-labels", type=int, default=256)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--stride", type=int, default=8, help="fine labels per coarse label")
    ap.add_argument("--passes", type=int, default=30)
    ap.add_argument("--slope", type=float, default=0.05)
    ap.add_argument("--trunc-labels", type=int, default=12, help="the truncated-linear potential is cut at that many labels (two-level, windows)")
    ap.add_argument("--full", action="store_true", help="two-level: also solve the full-range DIFF model")
    ap.add_argument("--order", default="colour_major", choices=["colour_major", "row_major"])
    ap.add_argument("--mode", default="anisotropic", choices=["anisotropic", "anisotropic2", "uniform", "damped_uniform"])
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("diff_shift_probe: no GPU", file=sys.stderr)
        return 2
    if a.compare + a.two_level + a.windows != 1:
        ap.error("one of --compare / --two-level / --windows")
    out = dict(mode_of_run="compare" if a.compare else "two-level" if a.two_level else "windows", grid=a.grid, order=a.order, mode=a.mode,
               device=torch.cuda.get_device_name(0))
    rc = compare(a, out) if a.compare else two_level(a, out) if a.two_level else windows(a, out)
    print(json.dumps(out))
    return rc


if __name__ == "__main__":
    sys.exit(main())
