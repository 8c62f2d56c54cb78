"""Every device format and every format choice of a fixed list of small operators equals a
recording (tests/golden/format_fingerprints.json): the digest of the CSR-block arrays
(format_digest) and the `info` fields that the template window, march shift, uniform-stencil
master, x-tile line width, kernel variant, byte counts and hybrid-GS structures decide.  A
change that only moves host code (the format builders of par_matrix.hip) leaves all of it as
it is; equality is asserted, nothing looser.

The operators are A, and A / P / R of every level, of the hierarchies in CASES; the last case
runs on two loopback ranks (boundary blocks, boundary slabs, the split agreement).  Where the
smoother is hybrid GS, every square operator takes one forward and one backward sweep at the
hierarchy's block size (64) before its `info` is read, so the GS fields are built.  At 64 rows
per chunk these grids' plane offsets (40; 29..31) fall inside a chunk, which rules GS templates
out, so the operator then takes the same two sweeps at GS_TPL_BLOCK = 8 and the GS fields are
recorded again under "gs_block8": a second build of the GS structures on the same operator,
with GS templates on the stencil levels (the template term in gs_bytes, no split) unless
AMG_GS_TEMPLATES=0 rules them out.

Re-recording, when a later change alters a format on purpose: build the library from the
commit whose formats are the new truth and run this module as a script on a GPU,

    python -m tests.test_gpu_format_fingerprints            # rewrites the fixture
    python -m tests.test_gpu_format_fingerprints OUT.json   # writes elsewhere (to compare)

The script records everything twice and refuses to write a fixture if the two recordings
differ (a field that is not deterministic cannot be pinned).  Say in the change why the
recording moved."""
import contextlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "format_fingerprints.json")

FIELDS = ("n_blocks", "n_vi_blocks", "n_templates", "template_rows",
          "tpl_window", "tpl_lanes", "tpl_march_shift", "tpl_master",
          "tile_line_bytes", "kernel_variant",
          "spmv_bytes", "mult_add_bytes", "residual_bytes", "jacobi_bytes", "gs_bytes",
          "gs_split", "gs_chain_maxw")

GS_FIELDS = ("gs_bytes", "gs_split", "gs_chain_maxw")
GS_TPL_BLOCK = 8  # in-chunk offsets of the 7-pt / 27-pt stencils are +-1 only: GS templates apply

# name: (ranks, stencil, grid, coarsening, smoother, environment of the build)
CASES = {
    "7pt-pmis-jacobi": (1, "7pt", (40, 36, 44), "pmis", "jacobi", {}),
    "27pt-sa-gs": (1, "27pt", (30, 28, 26), "sa", "hybrid_gs", {}),
    "5pt-pmis-jacobi": (1, "5pt", (300, 280), "pmis", "jacobi", {}),
    "7pt-lines32": (1, "7pt", (40, 36, 44), "pmis", "jacobi", {"AMG_TILE_LINE": "4"}),
    "7pt-pmis-gs": (1, "7pt", (40, 36, 44), "pmis", "hybrid_gs", {}),
    "27pt-sa-gs-no-gs-templates": (1, "27pt", (30, 28, 26), "sa", "hybrid_gs", {"AMG_GS_TEMPLATES": "0"}),
    "27pt-sa-gs-split-forced": (1, "27pt", (30, 28, 26), "sa", "hybrid_gs", {"AMG_GS_SPLIT_NPR": "0"}),
    "7pt-rect-tile-0": (1, "7pt", (40, 36, 44), "pmis", "jacobi", {"AMG_RECT_TILE": "0"}),
    "7pt-rect-tile-1": (1, "7pt", (40, 36, 44), "pmis", "jacobi", {"AMG_RECT_TILE": "1"}),
    "7pt-pmis-gs-2ranks": (2, "7pt", (40, 36, 44), "pmis", "hybrid_gs", {}),
}


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _fingerprint(ctx, M, sweeps):
    from tests.util import to_dev

    digest = M.format_digest()  # builds a deferred level operator; info alone does not

    def sweep(block):
        M.hybrid_gs(x, b, y, block=block)
        M.hybrid_gs(x, b, y, block=block, backward=True)
        ctx.synchronize()
        return M.info

    if sweeps:
        n = M.local_rows
        x, b, y = to_dev(ctx, np.zeros(n)), to_dev(ctx, np.ones(n)), to_dev(ctx, np.zeros(n))
        inf = sweep(64)
    else:
        inf = M.info
    out = {"digest": f"{digest:016x}"}
    out.update({k: int(inf[k]) for k in FIELDS})
    if sweeps:
        inf = sweep(GS_TPL_BLOCK)
        out["gs_block8"] = {k: int(inf[k]) for k in GS_FIELDS}
    return out


def _hierarchy(ctx, kind, dims, coarsen, smoother):
    import raptor_amd as ra

    gs = smoother == "hybrid_gs"
    A = ra.par_stencil_grid(ctx, kind, dims)
    ml = ra.ParMultilevel(coarsen=coarsen, smoother=smoother).setup(A)
    out = {"A": _fingerprint(ctx, A, gs)}
    for l in range(ml.num_levels):
        out[f"A{l}"] = _fingerprint(ctx, ml.level_matrix(l, "A"), gs)
        if l + 1 < ml.num_levels:
            out[f"P{l}"] = _fingerprint(ctx, ml.level_matrix(l, "P"), False)
            out[f"R{l}"] = _fingerprint(ctx, ml.level_matrix(l, "R"), False)
    return out


def record(name):
    """The fingerprints of one case: {operator: {field: value}}, per rank for a loopback case."""
    from tests.util import loopback_ctx, make_ctx

    ranks, kind, dims, coarsen, smoother, env = CASES[name]
    with _environment(env):
        if ranks == 1:
            return _hierarchy(make_ctx(0), kind, dims, coarsen, smoother)
        from tests.test_gpu_multirank import run_ranks

        res = run_ranks(ranks, lambda r, nr, world: _hierarchy(loopback_ctx(r, nr, world), kind, dims,
                                                               coarsen, smoother))
        return {f"rank{r}": res[r] for r in range(ranks)}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_formats_equal_recording(name, recorded):
    got = record(name)
    want = recorded[name]
    assert sorted(got) == sorted(want)
    for op in want:  # per operator first: a failure names the operator and the field
        assert got[op] == want[op], (name, op)
    assert got == want


if __name__ == "__main__":
    first = {name: record(name) for name in CASES}
    second = {name: record(name) for name in CASES}
    if first != second:
        for name in CASES:
            if first[name] != second[name]:
                print("not deterministic:", name, file=sys.stderr)
                print(json.dumps(first[name], indent=1), json.dumps(second[name], indent=1), file=sys.stderr)
        sys.exit("two recordings differ: no fixture written")
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(first, f, indent=1, sort_keys=True)
        f.write("\n")
    n_ops = sum(len(v) if "A" in v else sum(len(r) for r in v.values()) for v in first.values())
    print(f"recorded {n_ops} operators of {len(first)} cases -> {path}")
