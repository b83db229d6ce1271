#!/usr/bin/env python3
"""tools/kernel_ab_probe.py NAME=DIR [NAME=DIR ...] — several builds of the library against one another on the workloads whose kernels
the fold of the copied kernel bodies touched (EXPERIMENTS.md P): same bits, same time?

DIR is a directory that holds ``lp_mp_amd/`` and ``include/`` with the library already built (the repository root, or
``git archive REV lp_mp_amd include`` unpacked somewhere and built with ``python -c "import lp_mp_amd.build as b; b.build()"`` from
there).  Give the baseline twice (two builds of the same source, named ``parent`` and ``parent2``): their per-round medians are the
spread a build named ``tree`` is judged by.  Every round starts one fresh child process per build (PYTHONPATH=DIR), the builds
taking turns; a child that does not exit 0 ends the run.  Per workload and child: one timed pass for the kernel names, SAMPLES
samples of WARM warm-up + STEPS timed passes ending in a device synchronise, lower_bound() / factor_lower_bounds() after one more
pass each, lower_bound() after lpmp_set_constants made a tenth of the pairwise factors stale (the list kernel), then sha256 of the
duals, the bound as hex and sha256 of the per-factor bounds.  Writes OUT/kernel_fold_parent_vs_tree.json and one .jsonl per child.

    python tools/kernel_ab_probe.py --rounds 9 --out OUT parent=/tmp/parent parent2=/tmp/parent2 tree=."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

SAMPLES, WARM, STEPS = 5, 3, 6


def diff_vectors(potential, L, T, seed):
    import numpy as np
    from lp_mp_amd import model as M, synthetic as S
    K = L // 4
    if potential == "linear":
        return np.stack([M.truncated_linear(L, L, 0.02 * (t + 1), 0.02 * (t + 1) * K) for t in range(T)])
    return S.u01(T * (2 * L - 1), seed + 1000).reshape(T, 2 * L - 1)


def right_grid(H, W, L, seed):
    import numpy as np
    from lp_mp_amd import model as M, synthetic as S
    mt = [M.MsgType(0, 1, M.SCHED_RIGHT, 0, 1, M.M_UNARY_PAIRWISE, 0), M.MsgType(0, 1, M.SCHED_RIGHT, 0, 1, M.M_UNARY_PAIRWISE, 1)]
    b = M.ModelBuilder(2, mt)
    n = H * W
    var = S.grid_variable_order(H, W, "colour_major").reshape(-1)
    a, bb = S.grid_edges(H, W)
    i, j = np.minimum(var[a], var[bb]), np.maximum(var[a], var[bb])
    u = b.add_vector_factors(0, S.u01(n * L, seed).reshape(n, L))
    p = b.add_dense_pairwise(1, S.u01(len(a) * L * L, seed + 1).reshape(-1, L, L))
    b.add_interleaved_messages(np.tile(np.array([0, 1], np.int32), len(a)), np.stack([u[i], u[j]], 1).reshape(-1), np.repeat(p, 2))
    b.add_relations(np.stack([u[i], p], 1).reshape(-1), np.stack([p, u[j]], 1).reshape(-1))
    return b.finish()


def models():
    from lp_mp_amd import synthetic as S
    yield "diff_full_512x512_L128", lambda: S.grid_model(512, 512, 128, pairwise="diff", order="colour_major", seed=1, diff_tables=diff_vectors("random", 128, 2, 1)), None, {"diff"}
    yield "diff_band_512x512_L128", lambda: S.grid_model(512, 512, 128, pairwise="diff", order="colour_major", seed=1, diff_tables=diff_vectors("linear", 128, 2, 1)), None, {"diff"}
    for L, G in ((48, 128), (128, 48)):
        yield "dense_big_f64_%dx%d_L%d" % (G, G, L), lambda L=L, G=G: S.grid_model(G, G, L, order="colour_major", seed=1), None, {"dense_big"}
        yield "dense_big_f32_%dx%d_L%d" % (G, G, L), lambda L=L, G=G: S.grid_model(G, G, L, order="colour_major", seed=1).with_f32_tables(), "f32", {"dense_big"}
    yield "right_f64_256x256_L32", lambda: right_grid(256, 256, 32, 1), None, None
    yield "right_f32_256x256_L32", lambda: right_grid(256, 256, 32, 1).with_f32_tables(), "f32", None


def worker(OUT, ONLY):
    import numpy as np
    from lp_mp_amd import build as B, engine as E, model as M
    print(json.dumps(dict(library=E.library_path(), source_hash=B.source_hash())), flush=True)
    for name, make, prec, classes in models():
        if ONLY and name not in ONLY:
            continue
        m = make()
        e = E.Engine(0)
        if prec:
            e.upload(m, table_precision=prec)
        else:
            e.upload(m)
        e.set_reparametrization(M.REPAM_ANISOTROPIC)
        cls = [dict(e.plan.schedule_classes(d, M.REPAM_ANISOTROPIC)) for d in (0, 1)]
        if classes is not None:
            assert all(set(c) == classes for c in cls), cls
        e.enable_kernel_timing(True); e.reset_kernel_timing()
        e.compute_pass(1); e.synchronize()
        kt = e.kernel_timing(); e.enable_kernel_timing(False)
        kernels = sorted({v["kernel"].split("(")[0] for v in kt.values()})
        band = [e.plan.diff_band_info(d, M.REPAM_ANISOTROPIC) for d in (0, 1)] if name.startswith("diff") else None
        ms = []
        for _ in range(SAMPLES):
            e.compute_pass(WARM); e.synchronize()
            t0 = time.perf_counter()
            e.compute_pass(STEPS); e.synchronize()
            ms.append((time.perf_counter() - t0) / STEPS * 1e3)
        # lower_bound() after a pass that leaves the bounds of the factors that were sent to stale (factor_lb_list_kernel), and
        # every factor's bound recomputed (factor_lb_kernel)
        lb_ms, flb_ms = [], []
        for _ in range(SAMPLES):
            e.compute_pass(1); e.synchronize()
            t0 = time.perf_counter(); lb = e.lower_bound(); e.synchronize(); lb_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); flb = e.factor_lower_bounds(); e.synchronize(); flb_ms.append((time.perf_counter() - t0) * 1e3)
        d = e.download_duals()
        lb = e.lower_bound()
        stale_equal = bool(np.float64(lb).tobytes() == np.float64(e.lower_bound()).tobytes())
        # a tenth of the pairwise factors get their own constants again (lpmp_set_constants marks their bounds stale): lower_bound()
        # then recomputes just those from the list (factor_lb_list_kernel)
        pw = np.flatnonzero(m.f_kind != M.F_VECTOR)[::10].astype(np.int32)
        off, size = m.const_offsets(), m.const_sizes()
        rows = np.zeros((len(pw), int(size[pw].max())))
        for i, f in enumerate(pw):
            rows[i, :size[f]] = m.const_data[off[f]:off[f] + size[f]]
        list_ms, list_n = [], []
        for _ in range(SAMPLES):
            e.set_constants(pw, rows); e.synchronize()
            t0 = time.perf_counter(); lb2 = e.lower_bound(); e.synchronize(); list_ms.append((time.perf_counter() - t0) * 1e3)
            list_n.append(int(e.lower_bound_recomputed()))
        assert all(n == len(pw) for n in list_n), (list_n, len(pw), m.n_factors)
        out = dict(workload=name, lb_list_ms=list_ms, lb_list_n=list_n[0], lb_after_list_hex=float(lb2).hex(), classes=cls, kernels=kernels, diff_band_info=band, ms_per_pass=ms, lower_bound_ms=lb_ms, factor_lower_bounds_ms=flb_ms,
                   passes=1 + SAMPLES * (WARM + STEPS) + SAMPLES, duals_sha256=hashlib.sha256(np.ascontiguousarray(d).tobytes()).hexdigest(),
                   duals_bytes=int(d.nbytes), lower_bound_hex=float(lb).hex(), factor_bounds_sha256=hashlib.sha256(np.ascontiguousarray(flb).tobytes()).hexdigest(),
                   nan_duals=bool(np.isnan(d).any()), lb_repeatable=stale_equal)
        print(json.dumps(out), flush=True)
        with open(OUT, "a") as fh:
            fh.write(json.dumps(out) + "\n")
        e.close()
        del m, d, flb


    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("builds", nargs="*", help="NAME=DIR")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="all", help="comma-separated workload names")
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default="kernel_ab_out")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    only = None if a.only == "all" else set(a.only.split(","))
    if a.worker:
        return worker(a.worker, only)
    BUILDS = {b.split("=", 1)[0]: os.path.abspath(b.split("=", 1)[1]) for b in a.builds}
    if not {"parent", "parent2", "tree"} <= set(BUILDS):
        sys.exit("builds: parent=DIR parent2=DIR tree=DIR")
    os.makedirs(a.out, exist_ok=True)
    runs = {b: [] for b in BUILDS}
    order = list(BUILDS.items())
    for r in range(a.rounds):
        k = r % len(order)
        for b, path in order[k:] + order[:k]:            # (no build is always the last of its round)
            f = os.path.join(a.out, "fold_%s_round%d.jsonl" % (b, r))
            if os.path.exists(f):
                os.remove(f)
            env = dict(os.environ, PYTHONPATH=path)
            env.pop("LPMP_ENGINE_SO", None)
            p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", f, "--only", a.only], env=env)
            print("round %d %s: exit %d" % (r, b, p.returncode), flush=True)
            if p.returncode != 0:
                sys.exit("child failed (%s, round %d, exit %d): nothing more is started" % (b, r, p.returncode))
            runs[b].append({j["workload"]: j for j in map(json.loads, open(f))})
    res, ok = {}, True

    def verdict(m):
        pp = m["parent"] + m["parent2"]
        lo, hi = min(pp), max(pp)
        t = statistics.median(m["tree"])
        return dict(parent_median=statistics.median(m["parent"]), parent2_median=statistics.median(m["parent2"]), spread=[lo, hi], tree_median=t,
                    tree_rounds=m["tree"], parent_rounds=m["parent"], parent2_rounds=m["parent2"], within=bool(lo <= t <= hi), not_slower=bool(t <= hi))
    for w in runs["tree"][0]:
        v = {k: verdict({b: [statistics.median(r[w][k]) for r in runs[b]] for b in ("parent", "parent2", "tree")})
             for k in ("ms_per_pass", "lower_bound_ms", "factor_lower_bounds_ms", "lb_list_ms")}
        bits = {k: sorted({r[w][k] for b in BUILDS for r in runs[b]}) for k in ("duals_sha256", "lower_bound_hex", "factor_bounds_sha256", "lb_after_list_hex")}
        same = all(len(x) == 1 for x in bits.values())
        ok = ok and same
        t = runs["tree"][0][w]
        res[w] = dict(pass_ms=v["ms_per_pass"], lower_bound_ms=v["lower_bound_ms"], factor_lower_bounds_ms=v["factor_lower_bounds_ms"], lb_list_ms=v["lb_list_ms"],
                      lb_list_n=t["lb_list_n"], same_bits=same, bits=bits, passes=t["passes"], duals_bytes=t["duals_bytes"], kernels=t["kernels"],
                      classes=t["classes"], diff_band_info=t["diff_band_info"])
        p = res[w]["pass_ms"]
        print("%-28s pass ms parent %.4f parent2 %.4f spread [%.4f, %.4f] tree %.4f %s | list lb ms spread [%.4f, %.4f] tree %.4f | bits %s" % (
            w, p["parent_median"], p["parent2_median"], *p["spread"], p["tree_median"], "within" if p["within"] else ("BELOW" if p["not_slower"] else "ABOVE"),
            *res[w]["lb_list_ms"]["spread"], res[w]["lb_list_ms"]["tree_median"], "same" if same else "DIFFER"), flush=True)
    json.dump(dict(command="python tools/kernel_ab_probe.py --rounds %d --only %s parent=... parent2=... tree=." % (a.rounds, a.only), rounds=a.rounds,
                   samples_per_round=SAMPLES, warmup_passes=WARM, timed_passes=STEPS, workloads=res),
              open(os.path.join(a.out, "kernel_fold_parent_vs_tree.json"), "w"), indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
