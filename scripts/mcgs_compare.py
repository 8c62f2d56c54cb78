#!/usr/bin/env python3
"""Multicolour Gauss-Seidel against hybrid GS and Chebyshev degree 2, in one process on one GPU.

For BASELINE.json configs[2] (27-pt anisotropic 256^3) and configs[4] (the offline G3_circuit
substitute, RCM order, coarse drop tolerance 0.005), both smoothed aggregation as bench.py
configures them, the script sets up the hierarchy once per smoother and then, after a warm-up of
every solver, alternates them `--repeats` times.  Per repeat and smoother it times `--steps`
V-cycles and `solve` and `pcg` to a relative residual of `--tol`; it reports every repeat, the
median and the spread (max - min) / median, the cycle / iteration counts, the setup time and, for
the multicolour smoother, colours, readiness rounds, sweep path and byte model per level.  The
numbers of one run compare with each other only.

With `--timeline` it also takes the in-graph timeline of a multicolour cycle (the per-sweep
marks of amg_solver_cycle_timeline).  The small-level threshold is measured by running the
script twice, AMG_MC_GS_WG_ROWS=0 (a launch per colour on every level) against the default.

    python scripts/mcgs_compare.py [--grid 256,256,256] [--g3 1225,1225] [--repeats 3] [--out profiles/mc_gs]

writes <out>/compare_sa27.json and <out>/compare_g3sub.json and prints one summary line each.
Torch-free (native context), like bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def variants(ra, drop_tol):
    sa = lambda **kw: ra.ParSmoothedAggregationSolver(drop_tol=drop_tol, **kw)  # noqa: E731
    return [("hybrid_gs", lambda: sa()),
            ("chebyshev-2", lambda: sa(smoother="chebyshev", cheby_degree=2)),
            ("mc_gs", lambda: sa(smoother="mc_gs"))]


def spread(v):
    med = statistics.median(v)
    return {"runs": [round(t, 6) for t in v], "median": round(med, 6),
            "spread_rel": round((max(v) - min(v)) / med, 4) if med > 0 else None}


def run_problem(ra, ctx, problem, args):
    if problem == "sa27":
        grid = tuple(int(v) for v in args.grid.split(","))
        A = ra.par_stencil_grid(ctx, "27pt", grid)
        drop_tol = 0.0
    else:
        grid = tuple(int(v) for v in args.g3.split(","))
        A, _ = ra.par_graph_laplacian(ctx, grid[0], grid[1], seed=1).reorder("rcm")
        drop_tol = 0.005
    n = A.local_rows
    xs = ra.vector_uniform(ctx, n, A.first_row, 42)
    b = ctx.empty(n)
    A.mult(xs, b)
    x = ctx.zeros(n)
    ctx.synchronize()

    def timed(fn):
        x.zero_()
        ctx.synchronize()
        t = time.perf_counter()
        res = fn()
        ctx.synchronize()
        return time.perf_counter() - t, res

    solvers = []
    for label, make in variants(ra, drop_tol):
        t = time.perf_counter()
        ml = make().setup(A)
        ctx.synchronize()
        setup_s = time.perf_counter() - t
        for _ in range(args.warmup):  # graph capture, first-use builds, clocks
            timed(lambda: ml.solve(x, b, max_iter=args.steps))
            timed(lambda: ml.pcg(x, b, max_iter=3))
        solvers.append(dict(label=label, ml=ml, setup_s=setup_s, cyc=[], solve=[], pcg=[]))
        print(f"[{problem}] {label}: setup {setup_s:.2f} s, {ml.num_levels} levels", file=sys.stderr, flush=True)
    for rep in range(args.repeats):
        for s in solvers:  # alternating: every repeat visits every smoother
            ml = s["ml"]
            t, _ = timed(lambda: ml.solve(x, b, max_iter=args.steps))
            s["cyc"].append(args.steps / t)
            t, (_, h) = timed(lambda: ml.solve(x, b, max_iter=args.max_iter, tol=args.tol))
            s["solve"].append(t)
            s["solve_n"] = (len(h) - 1, bool(h[-1] <= args.tol * h[0]))
            t, (_, h) = timed(lambda: ml.pcg(x, b, max_iter=args.max_iter, tol=args.tol))
            s["pcg"].append(t)
            s["pcg_n"] = (len(h) - 1, bool(h[-1] <= args.tol * h[0]))
    out = {"problem": problem, "grid": list(grid), "rows": n, "drop_tol": drop_tol, "tol_rel": args.tol,
           "steps": args.steps, "warmup_rounds": args.warmup, "repeats": args.repeats,
           "mc_gs_wg_rows_env": os.environ.get("AMG_MC_GS_WG_ROWS"),
           "what": "one process, one GPU; smoothers alternated per repeat after every solver's warm-up; "
                   "seconds are wall time around a device sync; spread_rel = (max - min) / median",
           "smoothers": {}}
    for s in solvers:
        ml = s["ml"]
        infos = [ml.level_info(l) for l in range(ml.num_levels)]
        o = out["smoothers"][s["label"]] = {
            "setup_s": round(s["setup_s"], 3),
            "levels": ml.num_levels,
            "level_rows": [i["n_global"] for i in infos],
            "vcycles_per_s": spread(s["cyc"]),
            "solve": {"cycles": s["solve_n"][0], "reached": s["solve_n"][1], "seconds": spread(s["solve"])},
            "pcg": {"iterations": s["pcg_n"][0], "reached": s["pcg_n"][1], "seconds": spread(s["pcg"])},
            "stored_bytes_per_cycle": int(sum(i["stored_bytes_per_cycle_local"] for i in infos)),
        }
        if s["label"] == "mc_gs":
            lev = []
            for l in range(ml.num_levels - 1):
                Al = ml.level_matrix(l, "A")
                lev.append(dict(ml.level_colours(l), rounds=Al.colour_rounds(), mc_gs_bytes=Al.info["mc_gs_bytes"],
                                gs_model_bytes=12 * Al.info["nnz_local"] + 36 * Al.local_rows))
            o["mc_levels"] = lev
            if args.timeline:
                ops, mode = ml.cycle_timeline(x, b, reps=args.timeline)
                o["timeline"] = {"in_graph": mode, "reps": args.timeline,
                                 "ops_us": [[name, round(us, 2)] for name, us in ops]}
    base = out["smoothers"]["hybrid_gs"]
    for s in solvers[1:]:
        o = out["smoothers"][s["label"]]
        o["vs_hybrid_gs"] = {
            "solve_seconds_ratio": round(o["solve"]["seconds"]["median"] / base["solve"]["seconds"]["median"], 4),
            "pcg_seconds_ratio": round(o["pcg"]["seconds"]["median"] / base["pcg"]["seconds"]["median"], 4)}
    for s in solvers:
        del s["ml"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--grid", default="256,256,256", help="configs[2]: the 27-point grid")
    ap.add_argument("--g3", default="1225,1225", help="configs[4]: the substitute's lattice")
    ap.add_argument("--problems", default="sa27,g3sub")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=400)
    ap.add_argument("--timeline", type=int, default=0, help="replays of the multicolour cycle's in-graph timeline")
    ap.add_argument("--suffix", default="", help="appended to the output file names")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_gs"))
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats must be >= 3 (the spread between repeats is part of the result)")
    import raptor_amd as ra

    ctx = ra.Context.native(0)
    os.makedirs(args.out, exist_ok=True)
    for problem in args.problems.split(","):
        res = run_problem(ra, ctx, problem, args)
        path = os.path.join(args.out, f"compare_{problem}{args.suffix}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"problem": problem, "file": os.path.relpath(path, ROOT), **{
            k: {"vcycles_per_s": v["vcycles_per_s"]["median"], "solve": [v["solve"]["cycles"], v["solve"]["seconds"]["median"]],
                "pcg": [v["pcg"]["iterations"], v["pcg"]["seconds"]["median"]], "setup_s": v["setup_s"]}
            for k, v in res["smoothers"].items()}}), flush=True)


if __name__ == "__main__":
    main()
