#!/usr/bin/env python3
"""Times a re-solve of ONE structure with new costs: what the engine offered before (a fresh upload, which plans everything again)
against lpmp_upload_costs on the engine that solved instance 1 (nothing is planned).  GPU only: there is no CPU path.

    python tools/recost_probe.py --grid 1024 --labels 32                      # the headline grid: dense tables, colour-major
    python tools/recost_probe.py --grid 1024 --labels 128 --pairwise diff     # difference-indexed factors, no tables

Instance 1 (costs A) is uploaded and run once, so that every schedule and the joined-pass launch of --passes passes exist.  Then,
for the costs B of another seed that lie in HOST arrays, the clock runs from "new costs in host arrays" to "first pass done"
(synchronised) and on to "--passes passes done":

  (a) fresh:   Engine.upload + set_reparametrization + prepare_passes + compute_pass(1) + compute_pass(passes - 1)   (a new engine)
  (b) recost:  Engine.upload_costs + compute_pass(1) + compute_pass(passes - 1)                                      (engine of instance 1)
  (c) device:  the unaries of B already on the device: set_vectors(all, replace) + zero_pairwise_duals + the same passes
               (constants as they are: a new cost volume with the smoothness term kept)

(a) and (b) must leave bit-identical duals; (b) and (c) must not build a schedule (Engine.schedules_built).  Writes
profiles/recost_probe_<shape>.json with the library's source hash and prints the same JSON line.

    python tools/recost_probe.py --grid 1024 --labels 128 --pairwise diff --pool      # new pool values (lpmp_upload_shared_pool)
    python tools/recost_probe.py --grid 1024 --labels 32 --listed 1000                # K listed tables (lpmp_set_constants)

--pool (shared / diff): after (b), the pool of another parameter set goes to the same engine — Engine.upload_shared_pool + first pass,
against the fresh upload of the model with that pool.  --listed K: K pairwise factors spread over the model get new constants —
Engine.set_constants + first pass, against Engine.upload_costs of the whole array with the same numbers.  Both are warm starts
(the duals stay), must leave the duals of the path they are compared with, and must not build a schedule; their figures go into
the same JSON ("pool", "listed").
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=1024, help="the grid is GRID x GRID")
    ap.add_argument("--labels", type=int, default=32)
    ap.add_argument("--pairwise", default="dense", choices=["dense", "diff", "shared", "potts"])
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--order", default="colour_major", choices=["colour_major", "row_major"])
    ap.add_argument("--mode", default="anisotropic", choices=["anisotropic", "anisotropic2", "uniform", "damped_uniform"])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--pool", action="store_true", help="also time a swap of the shared pool (shared / diff) against a fresh upload")
    ap.add_argument("--listed", type=int, default=0, metavar="K", help="also time set_constants of K pairwise factors against upload_costs of the whole array")
    ap.add_argument("--out", default=None, help="default: profiles/recost_probe_<shape>.json")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("recost_probe: no GPU", file=sys.stderr)
        return 2
    if a.pool and a.pairwise not in ("shared", "diff"):
        print("recost_probe: --pool needs --pairwise shared or diff", file=sys.stderr)
        return 2
    from lp_mp_amd import build as B, engine as E, model as M, synthetic as S
    mode = M.REPAM_NAMES[a.mode]
    kw = {}
    if a.pairwise == "diff":
        L = a.labels
        kw["diff_tables"] = np.stack([M.truncated_linear(L, L, 0.05, 1.0), M.truncated_linear(L, L, 0.02, 0.6)])
    t0 = time.perf_counter()
    A = S.grid_model(a.grid, a.grid, a.labels, pairwise=a.pairwise, order=a.order, seed=a.seed, **kw)
    # B: the same structure, other numbers — unaries of another seed, constants shifted (one pass over the 17 GB of the headline grid)
    n_vec = int(a.grid * a.grid * a.labels)
    dual_b = np.zeros_like(A.dual_data)
    dual_b[:n_vec] = S.u01(n_vec, a.seed + 1000)
    assert np.all(A.f_kind[: a.grid * a.grid] == M.F_VECTOR) and A.dual_offsets()[a.grid * a.grid] == n_vec
    const_b = A.const_data + 0.25
    import dataclasses
    Bm = dataclasses.replace(A, const_data=const_b, dual_data=dual_b, _keep=[])
    shape = "%dx%dx%d_%s_%s" % (a.grid, a.grid, a.labels, a.pairwise, a.order)
    out = dict(shape=shape, grid=a.grid, labels=a.labels, pairwise=a.pairwise, order=a.order, mode=a.mode, passes=a.passes,
               const_bytes=int(A.const_data.nbytes), dual_bytes=int(A.dual_data.nbytes), host_models_s=time.perf_counter() - t0,
               device=torch.cuda.get_device_name(0), source_hash=B.source_hash())

    def passes(e):
        e.compute_pass(1); e.synchronize()
        t1 = time.perf_counter()
        if a.passes > 1:
            e.compute_pass(a.passes - 1)
        e.synchronize()
        return t1, time.perf_counter()

    def fresh(model, n_passes=None):
        t = time.perf_counter()
        e = E.Engine(0)
        e.upload(model, rows_layout=False); e.set_reparametrization(mode)
        t_up = time.perf_counter()
        if n_passes == 1:                  # (the pool comparison: the first pass is the figure)
            e.compute_pass(1); e.synchronize()
            t1 = time.perf_counter()
            return e, dict(upload_and_weights_s=t_up - t, first_pass_done_s=t1 - t)
        e.prepare_passes(1); e.prepare_passes(max(1, a.passes - 1))
        t_prep = time.perf_counter()
        t1, tn = passes(e)
        return e, dict(upload_and_weights_s=t_up - t, prepare_passes_s=t_prep - t_up, first_pass_done_s=t1 - t, all_passes_done_s=tn - t)

    e, out["instance_1_fresh"] = fresh(A)                     # instance 1: what every path starts from
    built = e.schedules_built()
    # (b) new costs in host arrays -> the engine that ran instance 1
    t = time.perf_counter()
    e.upload_costs(const=Bm.const_data if Bm.const_data.shape[0] else None, duals=Bm.dual_data)
    t_up = time.perf_counter()
    t1, tn = passes(e)
    out["recost"] = dict(upload_costs_s=t_up - t, first_pass_done_s=t1 - t, all_passes_done_s=tn - t, schedules_built_before=built,
                         schedules_built_after=e.schedules_built(), lower_bound=e.lower_bound())
    d_recost = torch.from_numpy(e.download_duals())
    # (c) the unaries already on the device (one [H W, L] volume), constants kept
    vol = torch.from_numpy(A.dual_data[:n_vec]).cuda(); torch.cuda.synchronize()
    factors = np.arange(a.grid * a.grid, dtype=np.int32)
    t = time.perf_counter()
    e.set_vectors(factors, src_dev=vol.data_ptr(), src_stride=a.labels)
    e.zero_pairwise_duals()
    e.synchronize()
    t_up = time.perf_counter()
    t1, tn = passes(e)
    out["device_unaries"] = dict(set_vectors_and_zero_s=t_up - t, first_pass_done_s=t1 - t, all_passes_done_s=tn - t,
                                 schedules_built_after=e.schedules_built())
    del vol
    ok_new = True
    if a.pool:
        # new pool values on the engine (constants of B, duals as they are now) against a fresh upload of that model with that pool
        if a.pairwise == "diff":          # another truncation: other bands, still banded
            sh = np.stack([M.truncated_linear(L, L, 0.1, 1.0), M.truncated_linear(L, L, 0.04, 0.6)]).reshape(-1)
        else:
            sh = 0.125 + S.u01(A.sh_data.shape[0], a.seed + 2000)
        held = e.download_duals()
        t = time.perf_counter()
        e.upload_shared_pool(sh)
        t_up = time.perf_counter()
        e.compute_pass(1); e.synchronize()
        t1 = time.perf_counter()
        d_pool = torch.from_numpy(e.download_duals())
        out["pool"] = dict(pool_bytes=int(sh.nbytes), upload_shared_pool_s=t_up - t, first_pass_done_s=t1 - t, schedules_built_after=e.schedules_built())
        g, fr = fresh(dataclasses.replace(Bm.with_pool(sh), dual_data=held, _keep=[]), n_passes=1)
        out["pool"]["fresh"] = fr
        out["pool"]["duals_bit_identical"] = bool(torch.equal(torch.from_numpy(g.download_duals()), d_pool))
        out["pool"]["ratio_first_pass"] = fr["first_pass_done_s"] / out["pool"]["first_pass_done_s"]
        g.close(); del held, d_pool
        ok_new = ok_new and out["pool"]["duals_bit_identical"] and out["pool"]["schedules_built_after"] == built
    if a.listed > 0:
        # K pairwise factors spread over the model: listed rows against the whole packed array with the same numbers, same start
        pw = np.flatnonzero(A.f_kind != M.F_VECTOR)
        fs = np.unique(pw[np.linspace(0, len(pw) - 1, min(a.listed, len(pw))).astype(np.int64)]).astype(np.int32)
        coff = A.const_offsets()
        csz = int((coff[fs + 1] - coff[fs]).max())
        rows = 0.5 + S.u01(len(fs) * csz, a.seed + 3000).reshape(len(fs), csz)
        held = e.download_duals()
        t = time.perf_counter()
        e.set_constants(fs, rows)
        t_up = time.perf_counter()
        e.compute_pass(1); e.synchronize()
        t1 = time.perf_counter()
        d_listed = torch.from_numpy(e.download_duals())
        out["listed"] = dict(k=int(len(fs)), row_entries=csz, listed_bytes=int(rows.nbytes), set_constants_s=t_up - t, first_pass_done_s=t1 - t,
                             schedules_built_after=e.schedules_built())
        whole = np.array(Bm.const_data, copy=True)
        for i, f in enumerate(fs):
            whole[coff[f]:coff[f + 1]] = rows[i, :coff[f + 1] - coff[f]]
        e.upload_costs(duals=held)
        t = time.perf_counter()
        e.upload_costs(const=whole)
        t_up = time.perf_counter()
        e.compute_pass(1); e.synchronize()
        t1 = time.perf_counter()
        out["listed"]["whole_array"] = dict(upload_costs_s=t_up - t, first_pass_done_s=t1 - t)
        out["listed"]["duals_bit_identical"] = bool(torch.equal(torch.from_numpy(e.download_duals()), d_listed))
        out["listed"]["ratio_first_pass"] = out["listed"]["whole_array"]["first_pass_done_s"] / out["listed"]["first_pass_done_s"]
        del held, d_listed, whole
        ok_new = ok_new and out["listed"]["duals_bit_identical"] and out["listed"]["schedules_built_after"] == built
    e.close()
    # (a) the same instance 2 the way the parent offers it
    f, out["fresh"] = fresh(Bm)
    out["fresh"]["lower_bound"] = f.lower_bound()
    out["duals_bit_identical"] = bool(torch.equal(torch.from_numpy(f.download_duals()), d_recost))
    f.close()
    out["ratio_first_pass"] = out["fresh"]["first_pass_done_s"] / out["recost"]["first_pass_done_s"]
    out["ratio_all_passes"] = out["fresh"]["all_passes_done_s"] / out["recost"]["all_passes_done_s"]
    out["nothing_planned"] = out["recost"]["schedules_built_after"] == built and out["device_unaries"]["schedules_built_after"] == built
    if a.pool or a.listed > 0:
        shape += ("_pool" if a.pool else "") + ("_listed%d" % a.listed if a.listed > 0 else "")
        out["shape"] = shape
    path = a.out or os.path.join(ROOT, "profiles", "recost_probe_%s.json" % shape)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0 if out["duals_bit_identical"] and out["nothing_planned"] and ok_new else 1


if __name__ == "__main__":
    sys.exit(main())
