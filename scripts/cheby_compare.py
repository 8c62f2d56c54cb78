#!/usr/bin/env python3
"""Chebyshev smoother against the current smoothers, in one process on one GPU.

For BASELINE.json configs[2] (27-pt anisotropic 256^3, smoothed aggregation) and configs[1]
(7-pt Poisson 256^3, PMIS) the script sets up the hierarchy once per smoother -- the current one
(hybrid GS / Jacobi, as bench.py configures them) and Chebyshev of degree 2 and 3 at the default
fraction -- and then, after a warm-up of every solver, alternates them `--repeats` times.  Per
repeat and smoother it times `--steps` V-cycles (V-cycles/s) and `solve` and `pcg` to a relative
residual of `--tol`; it reports every repeat, the median and the spread (max - min) / median,
the cycle / iteration counts and the setup time.  The current smoother's numbers of the same run
are the baseline (figures from another box or run are not comparable).

    python scripts/cheby_compare.py [--grid 256,256,256] [--repeats 3] [--out profiles/cheby]

writes <out>/compare_sa27.json and <out>/compare_7pt.json and prints one summary line each.
Torch-free (native context), like bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def variants(ra, problem):
    """(label, solver factory): the current smoother first, then Chebyshev degree 2 and 3."""
    if problem == "sa27":
        base = ("hybrid_gs", lambda: ra.ParSmoothedAggregationSolver())
        cheb = lambda m: ra.ParSmoothedAggregationSolver(smoother="chebyshev", cheby_degree=m)
    else:
        base = ("jacobi", lambda: ra.ParRugeStubenSolver(coarsen="pmis"))
        cheb = lambda m: ra.ParRugeStubenSolver(coarsen="pmis", smoother="chebyshev", cheby_degree=m)
    return [base, ("chebyshev-2", lambda: cheb(2)), ("chebyshev-3", lambda: cheb(3))]


def spread(v):
    med = statistics.median(v)
    return {"runs": [round(t, 6) for t in v], "median": round(med, 6),
            "spread_rel": round((max(v) - min(v)) / med, 4) if med > 0 else None}


def run_problem(ra, ctx, problem, grid, args):
    A = ra.par_stencil_grid(ctx, "27pt" if problem == "sa27" else "7pt", grid)
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
    for label, make in variants(ra, problem):
        t = time.perf_counter()
        ml = make().setup(A)
        ctx.synchronize()
        setup_s = time.perf_counter() - t
        lam = ([ml.level_eig(l) for l in range(ml.num_levels - 1)] if label.startswith("chebyshev") else None)
        for _ in range(args.warmup):  # graph capture, first-use builds, clocks
            timed(lambda: ml.solve(x, b, max_iter=args.steps))
            timed(lambda: ml.pcg(x, b, max_iter=3))
        solvers.append(dict(label=label, ml=ml, setup_s=setup_s, lam=lam, cyc=[], solve=[], pcg=[]))
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
    out = {"problem": problem, "grid": list(grid), "rows": n, "tol_rel": args.tol, "steps": args.steps,
           "warmup_rounds": args.warmup, "repeats": args.repeats,
           "what": "one process, one GPU; smoothers alternated per repeat after every solver's warm-up; "
                   "seconds are wall time around a device sync; spread_rel = (max - min) / median",
           "smoothers": {}}
    for s in solvers:
        infos = [s["ml"].level_info(l) for l in range(s["ml"].num_levels)]
        out["smoothers"][s["label"]] = {
            "setup_s": round(s["setup_s"], 3),
            "levels": s["ml"].num_levels,
            "level_eig": s["lam"],
            "vcycles_per_s": spread(s["cyc"]),
            "solve": {"cycles": s["solve_n"][0], "reached": s["solve_n"][1], "seconds": spread(s["solve"])},
            "pcg": {"iterations": s["pcg_n"][0], "reached": s["pcg_n"][1], "seconds": spread(s["pcg"])},
            "stored_bytes_per_cycle": int(sum(i["stored_bytes_per_cycle_local"] for i in infos)),
        }
    base = out["smoothers"][solvers[0]["label"]]
    for s in solvers[1:]:
        o = out["smoothers"][s["label"]]
        o["vs_" + solvers[0]["label"]] = {
            "solve_seconds_ratio": round(o["solve"]["seconds"]["median"] / base["solve"]["seconds"]["median"], 4),
            "pcg_seconds_ratio": round(o["pcg"]["seconds"]["median"] / base["pcg"]["seconds"]["median"], 4)}
    for s in solvers:
        del s["ml"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--grid", default="256,256,256")
    ap.add_argument("--problems", default="sa27,7pt")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cheby"))
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats must be >= 3 (the spread between repeats is part of the result)")
    import raptor_amd as ra

    ctx = ra.Context.native(0)
    grid = tuple(int(v) for v in args.grid.split(","))
    os.makedirs(args.out, exist_ok=True)
    for problem in args.problems.split(","):
        res = run_problem(ra, ctx, problem, grid, args)
        path = os.path.join(args.out, f"compare_{problem}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"problem": problem, "file": os.path.relpath(path, ROOT), **{
            k: {"vcycles_per_s": v["vcycles_per_s"]["median"], "solve": [v["solve"]["cycles"], v["solve"]["seconds"]["median"]],
                "pcg": [v["pcg"]["iterations"], v["pcg"]["seconds"]["median"]], "setup_s": v["setup_s"]}
            for k, v in res["smoothers"].items()}}), flush=True)


if __name__ == "__main__":
    main()
