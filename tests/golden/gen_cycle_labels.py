"""tests/golden/cycle_labels.json: the operation order of one V-cycle, as the labels of
ParMultilevel.cycle_timeline(x, b, reps=1) without the trailing "event-node gap", on the 7-pt
28 x 26 x 24 grid for every smoother and sweep option tests/test_gpu_parity.py::
test_cycle_operation_order pins.  Needs a GPU and the built library.
Run: python tests/golden/gen_cycle_labels.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CONFIGS = [
    dict(coarsen="pmis", smoother="jacobi", pre_sweeps=1, post_sweeps=1),
    dict(coarsen="pmis", smoother="jacobi", pre_sweeps=2, post_sweeps=2),
    dict(coarsen="pmis", smoother="jacobi", pre_sweeps=0, post_sweeps=1),
    dict(coarsen="pmis", smoother="chebyshev", cheby_degree=3, pre_sweeps=1, post_sweeps=1),
    dict(coarsen="sa", smoother="hybrid_gs", pre_sweeps=1, post_sweeps=1),
    dict(coarsen="sa", smoother="hybrid_gs", pre_sweeps=2, post_sweeps=1),
    dict(coarsen="pmis", smoother="mc_gs", pre_sweeps=1, post_sweeps=1),
]


def main():
    import raptor_amd as ra

    ctx = ra.Context(0)
    A = ra.par_stencil_grid(ctx, "7pt", (28, 26, 24))
    n = A.local_rows
    out = []
    for cfg in CONFIGS:
        ml = ra.ParMultilevel(**cfg).setup(A)
        b = ra.vector_uniform(ctx, n, 0, 42)
        ops, _ = ml.cycle_timeline(ctx.zeros(n), b, reps=1)
        labels = [lab for lab, _ in ops if lab != "event-node gap"]
        out.append({"options": cfg, "labels": labels})
        print(cfg, len(labels))
    with open(os.path.join(HERE, "cycle_labels.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
