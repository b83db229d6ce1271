#!/usr/bin/env python3
"""Times lpmp_forest_moves (exact relabelling of induced forests given all other labels) next to lpmp_path_moves, the
decode's refinement sweep and a pass of the same engine, and continues the energy table of DESIGN.md 8.  GPU only.

    python tools/forest_moves_probe.py --n 2000000 --m 10000000           (the C4 shape: a random graph, 16 labels)
    python tools/forest_moves_probe.py --rows 1024 --cols 1024 --labels 32
    python tools/forest_moves_probe.py --skip graph,grid                   (the energy table alone)

Three timed models, each on one engine after --passes anisotropic passes and a decode:
  graph          the counter-based random graph G(n, m) of the C4 workload, --graph-labels labels, with the suggested cover
  grid_cover     the headline grid in colour-major order with the suggested cover (Plan.suggest_forests)
  grid_paths     the same grid and engine with forests_from_paths(grid_paths(...)): the path groups as forests
Per model: milliseconds (HIP events on the engine's stream around the call; median, min, max of --repeat) of one round, of every
group of a round on its own with its launches (up levels + down levels) and the milliseconds per level, the primal cost before and
after, and for scale decode_primal(0, 1) (a decode with one refinement sweep), decode_primal(0, 0), a plain pass and — on the
grid — one round of lpmp_path_moves.
The energy table (tests/decode_cases.py holds its models): on the 24 x 24 grids of DESIGN.md 8 in both orders and on
random_graph(), after 5 and 50 passes: the bound, the decode, + 3 refinement sweeps, + 1 to 3 rounds of path moves (grids only),
+ 1 to 3 rounds of forest moves with the suggested cover, all from the decode's labels.
Prints one JSON line with the library's source hash; --out writes it to a file."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    s = sorted(ms)
    return dict(median_ms=s[len(s) // 2], min_ms=s[0], max_ms=s[-1], ms=ms)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--m", type=int, default=10_000_000)
    ap.add_argument("--graph-labels", type=int, default=16)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--labels", type=int, default=32)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--skip", default="", help="comma-separated: graph, grid, table")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("forest_moves_probe: no GPU", file=sys.stderr)
        return 2
    from lp_mp_amd import build as B, engine as E, model as M, synthetic as S
    skip = set(a.skip.split(","))
    sp = torch.cuda.current_stream().cuda_stream
    out = dict(repeat=a.repeat, passes=a.passes, library_source_hash=B.source_hash(), device=torch.cuda.get_device_name(0))
    ok = True

    def timed(f, n, before=None):
        ms = []
        for i in range(n):
            if before:
                before()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); f(); t1.record(); t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return ms

    def device_tables(m, n_vars, n_edges, L):
        """dense tables generated in HBM as bench.py generates them: (buffers to keep, upload keywords)"""
        const = torch.empty(n_edges * L * L, dtype=torch.float64, device="cuda:0")
        E.synth_fill(const.data_ptr(), const.numel(), a.seed, n_vars * L, sp)
        torch.cuda.synchronize()
        return (const,), dict(const_dev=const.data_ptr())

    def engine(m, keep, kw):
        e = E.Engine(0)
        e.set_stream(sp)
        e.upload(m, keep=keep, **kw)
        e.set_reparametrization(M.REPAM_ANISOTROPIC)
        return e

    def forest_timing(e, groups):
        """one round and every group of it, from the labels of a fresh decode"""
        nonlocal ok
        t0 = time.perf_counter()
        fs = e.forest_set(groups)
        create_s = time.perf_counter() - t0
        singles = [e.forest_set([g]) for g in groups]
        fresh = lambda: e.decode_primal(0, 0)
        fresh()
        before = e.evaluate_primal()
        fs.move(1)                                        # warm-up
        r = stats(timed(lambda: fs.move(1), a.repeat, before=fresh))
        r.update(energy_before=before, energy_after=e.evaluate_primal(), consistent=e.check_primal_consistency(), create_s=create_s,
                 n_groups=fs.n_groups, n_trees=fs.n_trees, max_height=fs.max_height, scratch_bytes=fs.scratch_bytes,
                 structure=e.plan.forest_info(groups), nodes_per_group=[int(len(u)) for u, _ in groups])
        ok = ok and r["consistent"] and r["energy_after"] <= before + 1e-9 * max(1.0, abs(before))
        for rounds in (2, 3):
            fresh(); fs.move(rounds)
            r["energy_after_%d_rounds" % rounds] = e.evaluate_primal()
        for s in singles:
            s.move(1)                                     # warm-up
        fresh()
        per = []
        for s in singles:
            ms = timed(lambda: s.move(1), 1)[0]
            launches = 2 * s.max_height + 1               # up levels (height + 1; both forms of a level count as one) + down levels
            per.append(dict(ms=ms, max_height=s.max_height, n_trees=s.n_trees, levels=launches, ms_per_level=ms / launches))
        r["groups_of_round_1"] = per
        for s in singles:
            s.close()
        fs.close()
        return r

    def scale(e, r):
        e.decode_primal(0, 1)
        r["decode_refine_1"] = stats(timed(lambda: e.decode_primal(0, 1), a.repeat))
        r["decode_refine_1"]["energy"] = e.evaluate_primal()
        r["decode"] = stats(timed(lambda: e.decode_primal(0, 0), a.repeat))
        r["decode"]["energy"] = e.evaluate_primal()
        lb = e.lower_bound()
        r["plain_pass"] = stats(timed(lambda: e.compute_pass(1), a.repeat + 1)[1:])
        r["lower_bound"] = lb

    if "graph" not in skip:
        n, m_e, L = a.n, a.m, a.graph_labels
        t0 = time.perf_counter()
        m = S.counter_graph_model(n, m_e, L, a.seed, device_const=True)
        keep, kw = device_tables(m, n, m_e, L)
        e = engine(m, keep, kw)
        t1 = time.perf_counter()
        groups = e.plan.suggest_forests()
        r = dict(n=n, m=m_e, labels=L, build_and_upload_s=t1 - t0, suggest_forests_s=time.perf_counter() - t1)
        e.compute_pass(a.passes)
        r["forest_round"] = forest_timing(e, groups)
        scale(e, r)
        r["round_over_plain_pass"] = r["forest_round"]["median_ms"] / r["plain_pass"]["median_ms"]
        out["graph"] = r
        e.close()
        del keep
        torch.cuda.empty_cache()

    if "grid" not in skip:
        H, W, L = a.rows, a.cols, a.labels
        m = S.grid_model(H, W, L, order="colour_major", seed=a.seed, device_const=True, compute_primal=True)
        keep, kw = device_tables(m, H * W, len(S.grid_edges(H, W)[0]), L)
        e = engine(m, keep, kw)
        t1 = time.perf_counter()
        cover = e.plan.suggest_forests()
        r = dict(rows=H, cols=W, labels=L, order="colour_major", suggest_forests_s=time.perf_counter() - t1)
        paths = S.grid_paths(H, W, "colour_major")
        e.compute_pass(a.passes)
        r["grid_cover"] = forest_timing(e, cover)
        r["grid_paths"] = forest_timing(e, M.forests_from_paths(paths))
        ps = e.path_set(paths)
        fresh = lambda: e.decode_primal(0, 0)
        fresh(); ps.move(1)
        r["path_moves_round"] = stats(timed(lambda: ps.move(1), a.repeat, before=fresh))
        r["path_moves_round"]["energy_after"] = e.evaluate_primal()
        ok = ok and r["path_moves_round"]["energy_after"] == r["grid_paths"]["energy_after"]     # the same labels, bit for bit
        ps.close()
        scale(e, r)
        for k in ("grid_cover", "grid_paths", "path_moves_round"):
            r[k + "_over_plain_pass"] = r[k]["median_ms"] / r["plain_pass"]["median_ms"]
        out["grid"] = r
        e.close()
        del keep
        torch.cuda.empty_cache()

    if "table" not in skip:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import decode_cases as DC
        rows = []
        cases = [("grid 24x24 %s, %s" % (kind, order), DC.table_grid(kind, order), S.grid_paths(24, 24, order))
                 for kind in ("random", "truncated") for order in ("row_major", "colour_major")] + [("random_graph 60/150", DC.random_graph(), None)]
        for name, m, paths in cases:
            e = engine(m, (), {})
            cover = e.plan.suggest_forests()
            fs = e.forest_set(cover)
            ps = e.path_set(paths) if paths else None
            done = 0
            for passes in (5, 50):
                e.compute_pass(passes - done)
                done = passes
                row = dict(model=name, passes=passes, groups=len(cover), bound=e.lower_bound())
                e.decode_primal(0, 0); row["decode"] = e.evaluate_primal()
                e.decode_primal(0, 3); row["decode_3_sweeps"] = e.evaluate_primal()
                for what, s in (("path", ps), ("forest", fs)):
                    if s is None:
                        continue
                    e.decode_primal(0, 0)
                    prev = row["decode"]
                    for k in (1, 2, 3):
                        s.move(1)
                        row["%s_%d" % (what, k)] = e.evaluate_primal()
                        ok = ok and row["%s_%d" % (what, k)] <= prev + 1e-9 * max(1.0, abs(prev))
                        prev = row["%s_%d" % (what, k)]
                rows.append(row)
            fs.close()
            if ps:
                ps.close()
            e.close()
        out["energy_table"] = rows

    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
