#!/usr/bin/env python3
"""FGMRES against solve, pcg and bicgstab, in one process on one GPU.

Two problems under PMIS + Jacobi (bench.py's configs[1] solver), as scripts/bicgstab_compare.py:
`convdiff` of tests/bicgstab_cases.py at cell Peclet number `--pe` on the `--grid` cube
(nonsymmetric: pcg is left out) and the 7-pt Poisson cube (symmetric).  After a warm-up of every
method the script alternates them `--repeats` times and reports, per method, the iterations (for
solve: cycles), the V-cycles spent and the wall time to a relative residual of `--tol` (every
repeat, the median, the spread (max - min) / median).  fgmres runs at every restart of
`--restarts`.

    python scripts/fgmres_compare.py [--grid 256,256,256] [--out profiles/fgmres]

writes <out>/compare_convdiff.json and <out>/compare_7pt.json and prints one summary line each.

Kernel bandwidths come from a kernel trace of a short eager run of this script:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \\
        python scripts/fgmres_compare.py --trace-run [--grid ...]
    python scripts/fgmres_compare.py --kernels DIR/.../run_kernel_trace.csv [--grid ...]

The trace run makes two eager fgmres calls of TRACE_ITERS iterations in one cycle (so launch k of
the dots and update kernels in a call is column j = k) and 20 amg_vector_copy / amg_vector_read
passes; --kernels takes the second call and prints (and writes <out>/kernels.json) per kernel the
time and the achieved bytes/s on the byte model (j + 2) 8n for the dots, (j + 3) 8n for the
update, 24n for the scale, (J + 2) 8n for the x update -- per column for the first two, and over
all launches -- against the copy and read passes of the same process.

That nothing waits for the host with tol == 0 is read off a HIP API trace:

    rocprofv3 --hip-trace --output-format csv -d DIR -o run -- \\
        python scripts/fgmres_compare.py --sync-run [--grid ...]
    python scripts/fgmres_compare.py --api DIR/.../run_hip_api_trace.csv

--sync-run makes one call that captures the graphs and a second that replays them; --api finds the
last unbroken run of hipGraphLaunch calls of the trace, which must be that whole second call (one
restart launch, SYNC_ITERS steps, one closing restart launch), and names the API calls on either
side of it.  Torch-free (native context), like bench.py."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRACE_ITERS = 30   # one cycle of 30 columns
SYNC_ITERS = 20
NEW = ["fgmres_dots_kernel", "fgmres_update_kernel", "fgmres_scale_kernel", "fgmres_x_kernel"]
REF = {"copy_kernel": 2, "read_kernel": 1}   # amg_vector_copy, amg_vector_read: vectors of 8 n bytes


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
    # method -> (call returning the history, V-cycles per iteration)
    methods = {"solve": (lambda: ml.solve(x, b, max_iter=args.max_iter, tol=args.tol)[1], 1)}
    if symmetric:
        methods["pcg"] = (lambda: ml.pcg(x, b, max_iter=args.max_iter, tol=args.tol)[1], 1)
    methods["bicgstab"] = (lambda: ml.bicgstab(x, b, max_iter=args.max_iter, tol=args.tol)[1], 2)
    for m in sorted((int(v) for v in args.restarts.split(",")), reverse=True):   # largest first: one workspace
        methods["fgmres(%d)" % m] = (lambda m=m: ml.fgmres(x, b, max_iter=args.max_iter, tol=args.tol, restart=m)[1], 1)
    for _ in range(args.warmup):
        for fn, _ in methods.values():
            timed(fn)
    runs = {k: [] for k in methods}
    last = {}
    for _ in range(args.repeats):
        for k, (fn, _) in methods.items():
            t, h = timed(fn)
            runs[k].append(t)
            last[k] = h
    # fgmres reports the Arnoldi estimate: the true residual of its last x, by a solve of no cycles
    true_rel = {}
    for k, (fn, _) in methods.items():
        if k.startswith("fgmres"):
            x.zero_()
            h = fn()
            true_rel[k] = float(ml.solve(x, b, max_iter=0)[1][0] / h[0])
    out = {"problem": problem, "grid": list(grid), "rows": n, "tol_rel": args.tol,
           "pe": None if symmetric else args.pe, "symmetric": symmetric, "setup_s": round(setup_s, 3),
           "levels": ml.num_levels, "warmup_rounds": args.warmup, "repeats": args.repeats,
           "what": "one process, one GPU, PMIS + Jacobi; methods alternated per repeat after a warm-up "
                   "of each; seconds are wall time around a device sync; spread_rel = (max - min) / median; "
                   "fgmres' last_rel_residual is the Arnoldi estimate, true_rel_residual ||b - A x|| / ||b - A x_0||",
           "methods": {}}
    for k, (_, per_it) in methods.items():
        h = last[k]
        rel = float(h[-1] / h[0])
        out["methods"][k] = {"iterations": len(h) - 1, "cycles": per_it * (len(h) - 1), "reached": bool(rel < args.tol),
                             "last_rel_residual": rel, "seconds": spread(runs[k])}
        if k in true_rel:
            out["methods"][k]["true_rel_residual"] = true_rel[k]
    return out


def _problem_7pt(ra, ctx, grid, graph):
    A = ra.par_stencil_grid(ctx, "7pt", grid)
    n = A.local_rows
    xs = ra.vector_uniform(ctx, n, A.first_row, 42)
    b = ctx.empty(n)
    A.mult(xs, b)
    return A, n, b, ctx.zeros(n), ra.ParRugeStubenSolver(coarsen="pmis", use_graph=graph).setup(A)


def trace_run(ra, ctx, grid):
    """Eager launches for a kernel trace: two fgmres calls of one cycle, copy and read passes."""
    A, n, b, x, ml = _problem_7pt(ra, ctx, grid, False)
    for _ in range(2):
        x.zero_()
        ml.fgmres(x, b, max_iter=TRACE_ITERS, restart=TRACE_ITERS)
    part = ctx.empty(4 * ((n + 2047) // 2048))
    for _ in range(20):
        ra.vector_copy(ctx, b, x)
        ra.vector_read(ctx, b, part)
    ctx.synchronize()
    print(json.dumps({"trace_run": True, "rows": n}), flush=True)


def sync_run(ra, ctx, grid):
    """A capturing call, then a replaying call with tol == 0 for a HIP API trace."""
    A, n, b, x, ml = _problem_7pt(ra, ctx, grid, True)
    for _ in range(2):
        x.zero_()
        ctx.synchronize()
        ml.fgmres(x, b, max_iter=SYNC_ITERS, restart=30)
    print(json.dumps({"sync_run": True, "rows": n}), flush=True)


def kernels(path, n, out_dir):
    dur = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].replace("amg::(anonymous namespace)::", "").split("(")[0].split("<")[0]
        if name in NEW or name in REF:
            dur.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    m = TRACE_ITERS
    res = {"rows": n, "what": "kernel times (us) of the second eager fgmres call of a kernel trace, one cycle of "
                              "%d columns; bytes on the model 8 n per vector read or written, each counted once; "
                              "ratios against amg_vector_copy / amg_vector_read of the same process" % m,
           "kernels": {}}
    k = res["kernels"]
    for name, vec in REF.items():
        v = dur[name][len(dur[name]) // 4:]   # the first launches warm the caches and clocks
        us = sum(v) / len(v)
        k[name] = {"calls": len(v), "mean_us": round(us, 2), "TB_per_s": round(8 * n * vec / us / 1e6, 3)}

    def entry(us, vectors):
        tb = 8 * n * vectors / us / 1e6
        return {"us": round(us, 2), "vectors": vectors, "TB_per_s": round(tb, 3),
                "vs_copy": round(tb / k["copy_kernel"]["TB_per_s"], 3), "vs_read": round(tb / k["read_kernel"]["TB_per_s"], 3)}

    for name, extra in (("fgmres_dots_kernel", 2), ("fgmres_update_kernel", 3)):
        v = dur[name]
        assert len(v) == 2 * m, (name, len(v))
        v = v[m:]
        k[name] = {"per_column": {str(j): entry(v[j], j + extra) for j in (0, 1, 3, 7, 15, m - 1)},
                   "all_columns": entry(sum(v), sum(j + extra for j in range(m)))}
    v = dur["fgmres_scale_kernel"]
    # per call m + 2 launches: v_0, v_1 .. v_{m-1}, then two that return at once (v_m is never
    # formed; the closing restart finds the flag set)
    assert len(v) == 2 * (m + 2), len(v)
    k["fgmres_scale_kernel"] = dict(entry(sum(v[m + 2:2 * m + 2]) / m, 3), calls=m)
    v = dur["fgmres_x_kernel"]
    assert len(v) == 4, len(v)       # per call: the opening launch (J = 0, returns at once), the closing one
    k["fgmres_x_kernel"] = dict(entry(v[3], m + 2), J=m)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "kernels.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


def api(path, out_dir):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Function"] for r in rows]
    last = max(i for i, f in enumerate(names) if f == "hipGraphLaunch")
    first = last
    while first > 0 and names[first - 1] == "hipGraphLaunch":
        first -= 1
    res = {"what": "HIP API calls of the replaying fgmres call (tol == 0, %d iterations, restart 30): the last unbroken "
                   "run of hipGraphLaunch in the trace, and the calls on either side" % SYNC_ITERS,
           "graph_launches_back_to_back": last - first + 1, "expected": SYNC_ITERS + 2,
           "calls_before": names[max(0, first - 6):first], "calls_after": names[last + 1:last + 7]}
    res["no_host_wait_inside"] = res["graph_launches_back_to_back"] == res["expected"]
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "api_sync.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--grid", default="256,256,256")
    ap.add_argument("--problems", default="convdiff,7pt")
    ap.add_argument("--pe", type=float, default=2.0)
    ap.add_argument("--restarts", default="30,10")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fgmres"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--sync-run", action="store_true")
    ap.add_argument("--kernels", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--api", metavar="HIP_API_TRACE_CSV")
    args = ap.parse_args()
    grid = tuple(int(v) for v in args.grid.split(","))
    if args.kernels:
        return kernels(args.kernels, grid[0] * grid[1] * grid[2], args.out)
    if args.api:
        return api(args.api, args.out)
    if args.repeats < 3:
        ap.error("--repeats must be >= 3 (the spread between repeats is part of the result)")
    import raptor_amd as ra

    ctx = ra.Context.native(0)
    if args.trace_run:
        return trace_run(ra, ctx, grid)
    if args.sync_run:
        return sync_run(ra, ctx, grid)
    os.makedirs(args.out, exist_ok=True)
    for problem in args.problems.split(","):
        res = run_problem(ra, ctx, problem, grid, args)
        path = os.path.join(args.out, f"compare_{problem}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"problem": problem, "file": os.path.relpath(path, ROOT), "rows": res["rows"],
                          **{k: [v["iterations"], v["seconds"]["median"], v["reached"]]
                             for k, v in res["methods"].items()}}), flush=True)


if __name__ == "__main__":
    main()
