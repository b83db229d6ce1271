#!/usr/bin/env python3
"""What does carrying the duals along buy when label windows move (lpmp_move_windows)?  GPU only: there is no CPU path.

    python tools/move_windows_probe.py --grid 256 --window 32

A GRID x GRID MRF tracks a label ramp (a disparity that grows from left to right) over two frames.  Every variable holds a window of
--window absolute labels centred on its ground truth; the unary cost of an absolute label is a truncated distance to the ground
truth plus noise that belongs to the absolute label; the edges are DIFF_SHIFT factors on one compact truncated-linear vector, the
shift of an edge being the difference of its two window origins.  Between the frames the ground truth drifts by 1 label in the left
half of the grid and by 2 in the right half, and the windows follow.

Frame 0 is solved with --solve passes (anisotropic weights, colour-major order).  From that state frame 1 is started three ways,
--track single passes are run with the bound after each, and the passes each start needs to reach a TARGET bound are counted — the
bound a cold start has after --ref passes, less tol relative, for every tol of --tols (null: not within --track passes):

    move   WindowSet.move(delta, cost_old, cost_new): duals and shifts carried along on the device
    warm   the parent's warm start: set_constants (the new shifts) + set_vectors(new - old window-relative costs, accumulate);
           the messages stay where they are, at the wrong absolute labels
    cold   upload_costs(constants, duals = the new costs)

and one move (device inputs) is timed against the parent's way of changing all shifts and unaries (set_constants + set_vectors from
device arrays): wall-clock time between two synchronisations of the engine's stream, --repeat calls after one warm-up, median / min
/ max in ms.  Prints one JSON line with the library's source hash; --out writes it to a file."""
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
    ap.add_argument("--grid", type=int, default=256, help="the grid is GRID x GRID")
    ap.add_argument("--window", type=int, default=32, help="labels per variable")
    ap.add_argument("--solve", type=int, default=30, help="passes on frame 0")
    ap.add_argument("--ref", type=int, default=60, help="passes of the cold start that define the target bound")
    ap.add_argument("--track", type=int, default=20, help="single passes after every start")
    ap.add_argument("--tols", default="1e-2,1e-3,1e-4,1e-5,1e-6")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("move_windows_probe: no GPU", file=sys.stderr)
        return 2
    import numpy as np
    from lp_mp_amd import build as B, engine as E, model as M, synthetic as S
    H = W = a.grid
    L = a.window
    n = H * W
    rng = np.random.default_rng(a.seed)
    var = S.grid_variable_order(H, W, "colour_major").reshape(-1)      # var[cell] = index of the cell's variable
    cell_of = np.empty(n, np.int64); cell_of[var] = np.arange(n)
    col = cell_of % W
    full = L + 3 * W // 8 + 8                                           # absolute labels 0 ... full - 1
    noise = 0.3 * rng.uniform(0, 1, (n, full))                          # belongs to the variable's ABSOLUTE label
    gt0 = L // 2 + (3 * col) // 8                                       # the ramp
    drift = np.where(col < W // 2, 1, 2)

    def frame(gt):
        """(window origins, window-relative unary costs [n, L]) of a frame"""
        c = np.clip(gt - L // 2, 0, full - L)
        lab = c[:, None] + np.arange(L)[None, :]
        return c, np.minimum(0.3 * np.abs(lab - gt[:, None]), 2.0) + np.take_along_axis(noise, lab, 1)
    c0, un0 = frame(gt0)
    c1, un1 = frame(gt0 + drift)
    delta = (c1 - c0).astype(np.int32)
    Dc, zero = M.truncated_linear_compact(0.25, 1.5)
    ea, eb = S.grid_edges(H, W)
    i, j = np.minimum(var[ea], var[eb]), np.maximum(var[ea], var[eb])
    n_e = i.shape[0]

    def model(c, un):
        return S.grid_model(H, W, L, pairwise="diff_shift", order="colour_major", seed=a.seed, unaries=un.reshape(-1), diff_tables=[Dc],
                            scales=np.ones(n_e), shifts=M.window_shift(c[i], c[j], zero))
    m0, m1 = model(c0, un0), model(c1, un1)
    us = np.flatnonzero(m0.f_kind == M.F_VECTOR).astype(np.int32)
    pw = np.flatnonzero(m0.f_kind != M.F_VECTOR).astype(np.int32)
    rows1 = m1.const_data.reshape(-1, 2)
    out = dict(grid=a.grid, window=L, absolute_labels=int(full), order="colour_major", weights="anisotropic", solve_passes=a.solve, ref_passes=a.ref,
               tols=a.tols, track=a.track, moved_unaries=int(np.count_nonzero(delta)), deltas=sorted(set(delta.tolist())),
               library_source_hash=B.source_hash(), device=torch.cuda.get_device_name(0))
    if n <= 1 << 16:      # (plain Python over every message: seconds at this size) the shifts a move writes are frame 1's
        assert M.move_windows(m0, m0.dual_data, us, delta)[0].const_data.tobytes() == m1.const_data.tobytes()
    e = E.Engine(0)
    e.upload(m0)
    e.set_reparametrization(M.REPAM_ANISOTROPIC)
    e.compute_pass(a.solve)
    d0 = e.download_duals()
    out["frame0_bound"] = e.lower_bound()
    ws = e.window_set(us)

    def restore():
        e.upload_costs(const=m0.const_data, duals=d0)

    def cold():
        e.upload_costs(const=m1.const_data, duals=m1.dual_data)

    def warm():
        e.set_constants(pw, rows1)
        e.set_vectors(us, un1 - un0, accumulate=True)

    def move():
        ws.move(delta, cost_old=un0, cost_new=un1)
    cold()
    e.compute_pass(a.ref)
    ref = e.lower_bound()
    tols = [float(t) for t in a.tols.split(",")]
    out["ref_bound"] = ref
    out["target_bounds"] = {"%g" % t: ref - t * abs(ref) for t in tols}
    for name, start in (("move", move), ("warm", warm), ("cold", cold)):
        restore()
        start()
        bounds = [e.lower_bound()]
        for _ in range(a.track):
            e.compute_pass(1)
            bounds.append(e.lower_bound())
        out[name] = dict(bounds=bounds, passes_to_target={"%g" % t: next((k for k, b in enumerate(bounds) if b >= ref - t * abs(ref)), None) for t in tols})

    # the time of a move against the parent's way of changing all shifts and all unaries, every input in device memory
    def wall(f):
        e.synchronize()
        t0 = time.perf_counter()
        f()
        e.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def series(f):
        wall(f)
        return stats([wall(f) for _ in range(a.repeat)])
    t_delta = torch.from_numpy(delta).cuda()
    t_zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    t_old, t_new, t_diff = torch.from_numpy(un0).cuda(), torch.from_numpy(un1).cuda(), torch.from_numpy(un1 - un0).cuda()
    t_rows = torch.from_numpy(np.ascontiguousarray(rows1)).cuda()
    torch.cuda.synchronize()
    restore()
    out["move_device_inputs"] = series(lambda: ws.move(delta_dev=t_delta.data_ptr(), cost_dev=(t_old.data_ptr(), t_new.data_ptr()), stride=L))
    out["move_device_delta_only"] = series(lambda: ws.move(delta_dev=t_delta.data_ptr()))
    out["move_zero_delta"] = series(lambda: ws.move(delta_dev=t_zero.data_ptr()))
    out["move_host_inputs"] = series(move)
    out["set_constants_plus_set_vectors_device"] = series(lambda: (e.set_constants(pw, src_dev=t_rows.data_ptr(), src_stride=2),
                                                                   e.set_vectors(us, src_dev=t_diff.data_ptr(), src_stride=L, accumulate=True)))
    out["set_constants_plus_set_vectors_host"] = series(warm)
    out["forward_pass"] = series(lambda: e.forward_pass())
    out["unaries"], out["pairwise"], out["dual_bytes"] = int(us.shape[0]), int(pw.shape[0]), int(m0.dual_sizes().sum()) * 8
    ws.close()
    e.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
