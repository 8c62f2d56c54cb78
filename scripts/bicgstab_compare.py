#!/usr/bin/env python3
"""BiCGStab against solve and pcg, in one process on one GPU.

Two problems under PMIS + Jacobi (bench.py's configs[1] solver): the 7-pt Poisson cube of
BASELINE.json configs[1] (symmetric: pcg's ground, one cycle per iteration against BiCGStab's
two) and `convdiff` of tests/bicgstab_cases.py (7-pt diffusion + first-order upwind convection)
at cell Peclet number `--pe` on the `--grid` cube, built on the host and uploaded with from_csr.
After a warm-up of every method the script alternates them `--repeats` times and reports, per
method, the iterations and wall time to a relative residual of `--tol` (every repeat, the
median, the spread (max - min) / median).  On a nonsymmetric operator pcg is capped at
`--pcg-cap` iterations and its last relative residual is reported instead.

Per BiCGStab iteration it also reports the time outside the two cycles and the two SpMVs: the
slope of bicgstab(max_iter = K) between K = 10 and K = 30 (tol = 0, graphs replayed back to back)
less two V-cycle replays and two `mult` calls timed the same way.

    python scripts/bicgstab_compare.py [--grid 256,256,256] [--out profiles/bicgstab]

writes <out>/compare_7pt.json and <out>/compare_convdiff.json and prints one summary line each.

Kernel bandwidths come from a kernel trace of a short eager run of this script:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \\
        python scripts/bicgstab_compare.py --trace-run [--grid ...]
    python scripts/bicgstab_compare.py --kernels DIR/.../run_kernel_trace.csv [--grid ...]

The trace run launches 20 BiCGStab and PCG iterations and 20 amg_vector_copy / amg_vector_read
passes over vectors of the same length; --kernels prints (and writes <out>/kernels.json) per
kernel the mean time, the bytes it moves (every vector read or written counted once) and the
achieved bytes/s against the copy and read passes of the same process.
Torch-free (native context), like bench.py."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# kernel -> vectors of 8 n bytes read + written
VECTORS = {"bicg_s_kernel": 3,       # r, v -> s
           "bicg_tsdot_kernel": 2,   # t, s
           "bicg_xr_kernel": 8,      # x, phat, shat, s, t, rhat -> x, r
           "bicg_p_kernel": 4,       # r, v, p -> p
           "pcg_xr_kernel": 6,       # p, q, x, r -> x, r
           "pcg_p_kernel": 3,        # z, p -> p
           "dot_partials_kernel": 2,
           "copy_kernel": 2,         # amg_vector_copy
           "read_kernel": 1}         # amg_vector_read


def spread(v):
    med = statistics.median(v)
    return {"runs": [round(t, 6) for t in v], "median": round(med, 6),
            "spread_rel": round((max(v) - min(v)) / med, 4) if med > 0 else None}


def build(ra, ctx, problem, grid, pe):
    if problem == "7pt":
        return ra.par_stencil_grid(ctx, "7pt", grid)
    from tests.bicgstab_cases import convdiff

    rp, col, val = convdiff(*grid, pe)
    return ra.ParCSRMatrix.from_csr(ctx, rp.size - 1, 0, rp, col, val)


def run_problem(ra, ctx, problem, grid, args):
    A = build(ra, ctx, problem, grid, args.pe)
    n = A.local_rows
    xs = ra.vector_uniform(ctx, n, A.first_row, 42)
    b = ctx.empty(n)
    A.mult(xs, b)
    x = ctx.zeros(n)
    y = ctx.empty(n)
    t = time.perf_counter()
    ml = ra.ParRugeStubenSolver(coarsen="pmis").setup(A)
    ctx.synchronize()
    setup_s = time.perf_counter() - t

    def timed(fn):
        x.zero_()
        ctx.synchronize()
        t = time.perf_counter()
        res = fn()
        ctx.synchronize()
        return time.perf_counter() - t, res

    symmetric = problem == "7pt"
    cap = args.max_iter if symmetric else args.pcg_cap
    methods = {"solve": lambda: ml.solve(x, b, max_iter=args.max_iter, tol=args.tol)[1],
               "pcg": lambda: ml.pcg(x, b, max_iter=cap, tol=args.tol)[1],
               "bicgstab": lambda: ml.bicgstab(x, b, max_iter=args.max_iter, tol=args.tol)[1:]}
    for _ in range(args.warmup):
        for fn in methods.values():
            timed(fn)
    runs = {k: [] for k in methods}
    last = {}
    for _ in range(args.repeats):
        for k, fn in methods.items():
            t, res = timed(fn)
            runs[k].append(t)
            last[k] = res
    out = {"problem": problem, "grid": list(grid), "rows": n, "tol_rel": args.tol,
           "pe": None if symmetric else args.pe, "symmetric": symmetric, "setup_s": round(setup_s, 3),
           "levels": ml.num_levels, "warmup_rounds": args.warmup, "repeats": args.repeats,
           "what": "one process, one GPU, PMIS + Jacobi; methods alternated per repeat after a warm-up "
                   "of each; seconds are wall time around a device sync; spread_rel = (max - min) / median",
           "methods": {}}
    for k in methods:
        h = last[k][0] if k == "bicgstab" else last[k]
        rel = float(h[-1] / h[0])
        out["methods"][k] = {"iterations": len(h) - 1, "reached": bool(rel < args.tol),
                             "last_rel_residual": rel, "seconds": spread(runs[k])}
    out["methods"]["bicgstab"]["status"] = int(last["bicgstab"][1])

    # the part of a BiCGStab iteration outside its two cycles and two SpMVs
    def per_call(fn, k_lo=10, k_hi=30):
        fn(k_lo)
        v = []
        for _ in range(args.repeats):
            lo, _ = timed(lambda: fn(k_lo))
            hi, _ = timed(lambda: fn(k_hi))
            v.append((hi - lo) / (k_hi - k_lo))
        return statistics.median(v)

    def cycles(k):
        for _ in range(k):
            ml.cycle(x, b)

    def mults(k):
        for _ in range(k):
            A.mult(b, y)

    it = per_call(lambda k: ml.bicgstab(x, b, max_iter=k))
    cyc = per_call(cycles)
    mv = per_call(mults)
    out["bicgstab_iteration"] = {
        "what": "slope of the wall time between 10 and 30 iterations / replays / calls (median of the repeats)",
        "iteration_us": round(it * 1e6, 2), "cycle_us": round(cyc * 1e6, 2), "spmv_us": round(mv * 1e6, 2),
        "outside_cycles_and_spmvs_us": round((it - 2 * cyc - 2 * mv) * 1e6, 2)}
    return out


def trace_run(ra, ctx, grid, args):
    """Eager launches for a kernel trace: BiCGStab, PCG, copy and read over n-vectors."""
    A = ra.par_stencil_grid(ctx, "7pt", grid)
    n = A.local_rows
    xs = ra.vector_uniform(ctx, n, A.first_row, 42)
    b = ctx.empty(n)
    A.mult(xs, b)
    x = ctx.zeros(n)
    ml = ra.ParRugeStubenSolver(coarsen="pmis", use_graph=False).setup(A)
    ml.bicgstab(x, b, max_iter=20)
    x.zero_()
    ml.pcg(x, b, max_iter=20)
    part = ctx.empty(4 * ((n + 2047) // 2048))
    for _ in range(20):
        ra.vector_copy(ctx, b, x)
        ra.vector_read(ctx, b, part)
    ctx.synchronize()
    print(json.dumps({"trace_run": True, "rows": n}), flush=True)


def kernels(path, n, out_dir):
    dur = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].replace("amg::(anonymous namespace)::", "").split("(")[0].split("<")[0]
        if name in VECTORS:
            dur.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    res = {"rows": n, "what": "mean kernel time of a kernel trace; bytes = 8 n per vector read or written, "
                              "each counted once; ratios against amg_vector_copy / amg_vector_read of the same process",
           "kernels": {}}
    for name, v in dur.items():
        v = v[len(v) // 4:]  # the first launches warm the caches and clocks
        us = sum(v) / len(v)
        res["kernels"][name] = {"calls": len(v), "mean_us": round(us, 2), "bytes": 8 * n * VECTORS[name],
                                "TB_per_s": round(8 * n * VECTORS[name] / us / 1e6, 3)}
    k = res["kernels"]
    for name, d in k.items():
        if "copy_kernel" in k:
            d["vs_copy"] = round(d["TB_per_s"] / k["copy_kernel"]["TB_per_s"], 3)
        if "read_kernel" in k:
            d["vs_read"] = round(d["TB_per_s"] / k["read_kernel"]["TB_per_s"], 3)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "kernels.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--grid", default="256,256,256")
    ap.add_argument("--problems", default="7pt,convdiff")
    ap.add_argument("--pe", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=400)
    ap.add_argument("--pcg-cap", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bicgstab"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernels", metavar="KERNEL_TRACE_CSV")
    args = ap.parse_args()
    grid = tuple(int(v) for v in args.grid.split(","))
    if args.kernels:
        kernels(args.kernels, grid[0] * grid[1] * grid[2], args.out)
        return
    if args.repeats < 3:
        ap.error("--repeats must be >= 3 (the spread between repeats is part of the result)")
    import raptor_amd as ra

    ctx = ra.Context.native(0)
    if args.trace_run:
        trace_run(ra, ctx, grid, args)
        return
    os.makedirs(args.out, exist_ok=True)
    for problem in args.problems.split(","):
        res = run_problem(ra, ctx, problem, grid, args)
        path = os.path.join(args.out, f"compare_{problem}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"problem": problem, "file": os.path.relpath(path, ROOT), "rows": res["rows"],
                          **{k: [v["iterations"], v["seconds"]["median"], v["reached"]]
                             for k, v in res["methods"].items()},
                          "bicgstab_iteration": res["bicgstab_iteration"]}), flush=True)


if __name__ == "__main__":
    main()
