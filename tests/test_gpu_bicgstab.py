"""Solver::bicgstab (raptor_amd/csrc/multilevel.hip, the bicg_* kernels of kernels.hip) and the
first nonsymmetric operators on the device, against the CPU oracle and the restatement of
tests/bicgstab_cases.py (checked on the CPU by tests/test_bicgstab_cpu.py).

Bars: every level's A, P, R and split of a convection-diffusion hierarchy equal the oracle's bit
for bit (device and host setup, 1 - 3 ranks) and one V-cycle is the oracle's; BiCGStab iterates
are bit-identical to the restatement run on the product's dot tree (alpha, omega and beta come
from dot products, so x has no allowance); history entries within SQRT_ULPS of np.sqrt(rr_k),
the allowance tests/test_gpu_cycle_options.py gives PCG for the same device sqrt."""
import numpy as np
import pytest

from tests import bicgstab_cases as B
from tests import cycle_option_cases as K
from tests.test_gpu_cycle_options import SQRT_ULPS
from tests.test_gpu_multirank import level_starts, run_ranks, set_oracle_cuts
from tests.util import loopback_ctx, same_csr, to_dev, to_host

pytestmark = pytest.mark.gpu

GRID_IDS = ["x".join(map(str, d)) for d in B.GRIDS]
# name: (family of cycle_option_cases.FAMILIES, extended+i interpolation)
SETUPS = {"pmis+jacobi": ("jacobi", False), "pmis+ext+i": ("jacobi", True), "sa+hybrid_gs": ("gs", False)}
FAMS = {"jacobi": "pmis+jacobi", "gs": "sa+hybrid_gs"}


def _options(O, setup, **over):
    """(oracle options, product options) of a setup, max_coarse = 32."""
    fam, ext = SETUPS[setup]
    okw = K.oracle_options(O, fam, max_coarse=B.MAX_COARSE)
    pkw = K.product_options(fam, max_coarse=B.MAX_COARSE)
    if ext:
        okw.update(interp=O.INTERP_EXT_I, p_max=4)
        pkw.update(interp="ext+i", p_max=4)
    pkw.update(over)
    return okw, pkw


def _within_ulps(h, want, ulps):
    return h.shape == want.shape and bool(np.all(np.abs(h - want) <= ulps * np.spacing(want)))


def _local(ra, ctx, csr, lo=0, hi=None):
    """Rows [lo, hi) of a (row_ptr, col, val) matrix as a ParCSRMatrix."""
    rp, col, val = csr
    n = rp.size - 1
    hi = n if hi is None else hi
    return ra.ParCSRMatrix.from_csr(ctx, n, lo, rp[lo:hi + 1] - rp[lo], col[rp[lo]:rp[hi]],
                                    val[rp[lo]:rp[hi]])


def _levels(ml):
    """This rank's rows of every level's operators and split: [(first_row, matrix)] per name."""
    out = []
    for l in range(ml.num_levels):
        d = {}
        for w in ("APR" if l + 1 < ml.num_levels else "A"):
            M = ml.level_matrix(l, w)
            d[w] = (M.first_row, M.to_scipy_local())
        if l + 1 < ml.num_levels:
            d["split"] = ml.level_split(l)
        out.append(d)
    return out


def _check_levels(lev, Ho, tag):
    assert len(lev) == Ho.num_levels >= 3, tag
    for l, d in enumerate(lev):
        for w in ("APR" if "P" in d else "A"):
            f, M = d[w]
            assert same_csr(M, Ho.matrix(l, w)[f:f + M.shape[0]]), (tag, l, w)
        if "split" in d:
            f, M = d["A"]
            assert np.array_equal(d["split"], Ho.split(l)[f:f + M.shape[0]]), (tag, l, "split")


_PROBLEMS = {}


def _problem(O, key):
    """key: (nx, ny, nz, pe), ("chain", n, pe) or "one-level".  csr, oracle matrix, b."""
    if key not in _PROBLEMS:
        if key == "one-level":
            csr = B.convdiff(5, 3, 2, 2.0)
        elif key[0] == "chain":
            csr = B.upwind_chain(*key[1:])
        else:
            csr = B.convdiff(*key)
        Ao = B.oracle_matrix(O, csr)
        b = B.rhs(O, Ao.shape[0])
        b.setflags(write=False)
        _PROBLEMS[key] = (csr, Ao, b)
    return _PROBLEMS[key]


_RESTATED = {}


def _restated(O, key, setup, max_iter, tol):
    """The one-rank restatement of a case, computed once: x, sqrt(rr), status, the hierarchy."""
    k = (key, setup, max_iter, tol)
    if k not in _RESTATED:
        _, Ao, b = _problem(O, key)
        Ho = O.Hierarchy(Ao, **_options(O, setup)[0])
        x, rr, st = B.bicgstab_restated(Ho, Ao, np.zeros(b.size), b, max_iter, tol, K.dot_tree)
        x.setflags(write=False)
        _RESTATED[k] = (x, np.sqrt(rr), st, Ho)
    return _RESTATED[k]


# ---- 1. nonsymmetric hierarchies on the device ------------------------------------------------
@pytest.mark.parametrize("setup", list(SETUPS))
@pytest.mark.parametrize("pe", [0.5, 8.0])
@pytest.mark.parametrize("dims", B.GRIDS, ids=GRID_IDS)
def test_nonsymmetric_hierarchy_and_cycle(ctx, oracle, dims, pe, setup):
    """setup_device 1 and 0: every level's A, P, R and split are the oracle's, and one V-cycle
    from x = 0 is the oracle's bit for bit."""
    import raptor_amd as ra

    O = oracle
    csr, Ao, b = _problem(O, dims + (pe,))
    okw, _ = _options(O, setup)
    Ho = O.Hierarchy(Ao, **okw)
    xo = Ho.cycle(np.zeros(b.size), b)
    A = _local(ra, ctx, csr)
    db = to_dev(ctx, b)
    for mode in (1, 0):
        ml = ra.ParMultilevel(**_options(O, setup, setup_device=mode)[1]).setup(A)
        _check_levels(_levels(ml), Ho, mode)
        dx = ctx.zeros(b.size)
        ml.cycle(dx, db)
        assert np.array_equal(to_host(ctx, dx), xo), mode


@pytest.mark.parametrize("setup", list(SETUPS))
@pytest.mark.parametrize("pe", [0.5, 8.0])
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("dims", B.GRIDS, ids=GRID_IDS)
def test_nonsymmetric_hierarchy_and_cycle_ranks(oracle, dims, nranks, pe, setup):
    """The same on loopback ranks with ragged cuts (levels distributed): each rank's rows."""
    import raptor_amd as ra

    O = oracle
    csr, Ao, b = _problem(O, dims + (pe,))
    n = b.size
    cuts = B.ragged_cuts(n, nranks)
    Ho = O.Hierarchy(Ao, **_options(O, setup)[0])

    def rank(r, nr, world):
        c = loopback_ctx(r, nr, world)
        lo, hi = cuts[r], cuts[r + 1]
        A = _local(ra, c, csr, lo, hi)
        db = to_dev(c, b[lo:hi])
        out = []
        for mode in (1, 0):
            ml = ra.ParMultilevel(**_options(O, setup, setup_device=mode, replicate_below=0)[1]).setup(A)
            dx = c.zeros(hi - lo)
            ml.cycle(dx, db)
            out.append((_levels(ml), to_host(c, dx), level_starts(ml)))
            del ml
        return out

    res = run_ranks(nranks, rank)
    set_oracle_cuts(Ho, [per_mode[0] for per_mode in res])
    xo = Ho.cycle(np.zeros(n), b)
    for r, per_mode in enumerate(res):
        for mode, (lev, x, starts) in zip((1, 0), per_mode):
            _check_levels(lev, Ho, (r, mode))
            assert starts == res[r][0][2]   # both setups cut the levels alike
            assert np.array_equal(x, xo[cuts[r]:cuts[r + 1]]), (r, mode)


# ---- 2. iterates --------------------------------------------------------------------------------
def _run(ra, ctx, csr, b, pkw, **kw):
    A = _local(ra, ctx, csr)
    ml = ra.ParMultilevel(**pkw).setup(A)
    dx = ctx.zeros(b.size)
    _, h, st = ml.bicgstab(dx, to_dev(ctx, b), **kw)
    return to_host(ctx, dx), h, st


@pytest.mark.parametrize("fam", list(FAMS))
@pytest.mark.parametrize("pe", B.PES)
@pytest.mark.parametrize("dims", B.GRIDS, ids=GRID_IDS)
def test_six_iterations_bit_exact(ctx, oracle, dims, pe, fam):
    import raptor_amd as ra

    O = oracle
    key = dims + (pe,)
    csr, Ao, b = _problem(O, key)
    xr, want, st_r, _ = _restated(O, key, FAMS[fam], 6, 0.0)
    assert st_r == B.KRYLOV_OK and want.shape == (7,)
    x, h, st = _run(ra, ctx, csr, b, _options(O, FAMS[fam])[1], max_iter=6)
    assert st == ra.AMG_KRYLOV_OK and len(h) == 7
    assert np.array_equal(x, xr)
    assert _within_ulps(h, want, SQRT_ULPS), (h, want)


@pytest.mark.parametrize("fam", list(FAMS))
@pytest.mark.parametrize("pe", B.PES)
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("dims", B.GRIDS, ids=GRID_IDS)
def test_six_iterations_bit_exact_ranks(oracle, dims, nranks, pe, fam):
    """Loopback ranks with ragged cuts: each rank's dot values come from its own rows and are
    added in rank order (two values per allgather for the fused pairs)."""
    import raptor_amd as ra

    O = oracle
    csr, Ao, b = _problem(O, dims + (pe,))
    n = b.size
    cuts = B.ragged_cuts(n, nranks)
    okw, pkw = _options(O, FAMS[fam], replicate_below=0)
    Ho = O.Hierarchy(Ao, **okw)

    def rank(r, nr, world):
        c = loopback_ctx(r, nr, world)
        lo, hi = cuts[r], cuts[r + 1]
        ml = ra.ParMultilevel(**pkw).setup(_local(ra, c, csr, lo, hi))
        dx = c.zeros(hi - lo)
        _, h, st = ml.bicgstab(dx, to_dev(c, b[lo:hi]), max_iter=6)
        return to_host(c, dx), h, st, level_starts(ml)

    res = run_ranks(nranks, rank)
    set_oracle_cuts(Ho, res)
    xr, rr, st_r = B.bicgstab_restated(Ho, Ao, np.zeros(n), b, 6, 0.0,
                                       lambda u, v: K.dot_tree(u, v, cuts))
    want = np.sqrt(rr)
    assert st_r == B.KRYLOV_OK and want.shape == (7,)
    for r, (x, h, st, _) in enumerate(res):
        assert st == ra.AMG_KRYLOV_OK
        assert np.array_equal(x, xr[cuts[r]:cuts[r + 1]]), r
        assert _within_ulps(h, want, SQRT_ULPS), (r, h, want)
        assert np.array_equal(h, res[0][1])   # every rank reports the same history


# ---- 3. stopping ----------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("fam", list(FAMS))
@pytest.mark.parametrize("pe", B.PES)
def test_tolerance_stops_at_the_restatements_iteration(ctx, oracle, pe, fam, graph):
    """tol = 1e-8, cap 40 (the CPU module checks that no history ratio of these runs comes within
    1 % of the tolerance): iterations, x and history are the restatement's."""
    import raptor_amd as ra

    O = oracle
    key = B.GRIDS[0] + (pe,)
    csr, Ao, b = _problem(O, key)
    xr, want, st_r, _ = _restated(O, key, FAMS[fam], 40, 1e-8)
    assert st_r == B.KRYLOV_OK and 1 < len(want) <= 16
    x, h, st = _run(ra, ctx, csr, b, _options(O, FAMS[fam], use_graph=graph)[1], max_iter=40, tol=1e-8)
    assert st == ra.AMG_KRYLOV_OK and len(h) == len(want)
    assert np.array_equal(x, xr)
    assert _within_ulps(h, want, SQRT_ULPS), (h, want)
    assert h[-1] / h[0] < 1e-8 and np.all(h[:-1] / h[0] >= 1e-8)


# ---- 4. dot-span boundaries -----------------------------------------------------------------------
@pytest.mark.parametrize("pe", [0.5, 8.0])
@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_chain_sizes_on_the_dot_spans_edges(ctx, oracle, n, pe):
    """tridiag(-1 - pe, 2 + pe, -1), pmis + jacobi (the SA cycle does not precondition these
    chains): six iterations bit-identical, one block to two blocks + 1 entry."""
    import raptor_amd as ra

    O = oracle
    key = ("chain", n, pe)
    csr, Ao, b = _problem(O, key)
    xr, want, st_r, _ = _restated(O, key, "pmis+jacobi", 6, 0.0)
    assert st_r == B.KRYLOV_OK and want.shape == (7,) and np.all(np.isfinite(want))
    x, h, st = _run(ra, ctx, csr, b, _options(O, "pmis+jacobi")[1], max_iter=6)
    assert st == ra.AMG_KRYLOV_OK
    assert np.array_equal(x, xr)
    assert _within_ulps(h, want, SQRT_ULPS), (h, want)


# ---- 5. graphs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", list(FAMS))
def test_graphs_reuse_and_pcg_in_between(ctx, oracle, fam):
    """Graphs on and off give the same bits; a second call on the same solver and buffers
    (graph reuse) equals the first; other x, b buffers afterwards are solved correctly; pcg
    between two bicgstab calls changes neither."""
    import raptor_amd as ra

    O = oracle
    key = B.GRIDS[0] + (8.0,)
    csr, Ao, b = _problem(O, key)
    n = b.size
    xr, want, _, Ho = _restated(O, key, FAMS[fam], 6, 0.0)
    b2 = O.vec_uniform(n, 11)
    xr2, rr2, st2 = B.bicgstab_restated(Ho, Ao, np.zeros(n), b2, 6, 0.0, K.dot_tree)
    A = _local(ra, ctx, csr)
    for graph in (True, False):
        ml = ra.ParMultilevel(**_options(O, FAMS[fam], use_graph=graph)[1]).setup(A)
        assert ml.graph_enabled == graph
        dx, db = ctx.zeros(n), to_dev(ctx, b)
        dx2, db2 = ctx.zeros(n), to_dev(ctx, b2)
        dp = ctx.zeros(n)
        for call in range(2):   # the second call replays the first call's graphs
            if call:
                _zero(ctx, dx)
            _, h, st = ml.bicgstab(dx, db, max_iter=6)
            assert st == ra.AMG_KRYLOV_OK
            assert np.array_equal(to_host(ctx, dx), xr), (graph, call)
            assert _within_ulps(h, want, SQRT_ULPS), (graph, call)
            if call == 0:
                h_first = h
                ml.pcg(dp, db, max_iter=3)   # its own graph slots and buffers
            else:
                assert np.array_equal(h, h_first)
        _, h, st = ml.bicgstab(dx2, db2, max_iter=6)   # other buffers: the graphs are recaptured
        assert st == st2 == ra.AMG_KRYLOV_OK
        assert np.array_equal(to_host(ctx, dx2), xr2), graph
        assert _within_ulps(h, np.sqrt(rr2), SQRT_ULPS), graph
        fresh = ra.ParMultilevel(**_options(O, FAMS[fam], use_graph=graph)[1]).setup(A)
        dq = ctx.zeros(n)
        _, hp = fresh.pcg(dq, db, max_iter=3)
        assert np.array_equal(to_host(ctx, dp), to_host(ctx, dq))   # pcg unchanged by bicgstab


def _zero(ctx, v):
    """v = 0 in place (the same device address), on the context's stream."""
    if getattr(ctx, "is_native", False):
        v.zero_()
        return
    import torch

    with torch.cuda.stream(ctx.stream):
        v.zero_()


# ---- 6. breakdown and contract ------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("tol", [0.0, 1e-8])
def test_exact_start_is_a_breakdown_that_leaves_x(ctx, oracle, tol, graph):
    """b = A x0 by the product's own mult: r is exactly 0, so rhat.v = 0 in the first iteration;
    with tol = 0 the nine replays after the stop change nothing."""
    import raptor_amd as ra

    O = oracle
    csr, Ao, _ = _problem(O, B.GRIDS[1] + (0.5,))
    n = Ao.shape[0]
    A = _local(ra, ctx, csr)
    ml = ra.ParMultilevel(**_options(O, "pmis+jacobi", use_graph=graph)[1]).setup(A)
    x0 = np.rint(8 * O.vec_uniform(n, 3))
    dx, db = to_dev(ctx, x0), ctx.zeros(n)
    A.mult(dx, db)
    assert not np.any(Ao.residual(x0, to_host(ctx, db)))
    _, h, st = ml.bicgstab(dx, db, max_iter=10, tol=tol)
    assert st == ra.AMG_KRYLOV_BREAKDOWN and h.tolist() == [0.0]
    assert np.array_equal(to_host(ctx, dx), x0)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("max_iter,tol", [(10, 0.0), (10, 1e-300), (3, 0.0)])
def test_one_level_run_against_the_restatement(ctx, oracle, max_iter, tol, graph):
    """30 rows under max_coarse = 32: the cycle is the coarse solve and the run ends in a
    breakdown before iteration 10 -- the replays after it (tol = 0) change nothing and append
    nothing; three iterations end with status OK."""
    import raptor_amd as ra

    O = oracle
    csr, Ao, b = _problem(O, "one-level")
    Ho = O.Hierarchy(Ao, **_options(O, "pmis+jacobi")[0])
    assert Ho.num_levels == 1
    xr, rr, st_r = B.bicgstab_restated(Ho, Ao, np.zeros(b.size), b, max_iter, tol, K.dot_tree)
    assert st_r == (B.KRYLOV_BREAKDOWN if max_iter == 10 else B.KRYLOV_OK) and len(rr) <= 7
    x, h, st = _run(ra, ctx, csr, b, _options(O, "pmis+jacobi", use_graph=graph)[1],
                    max_iter=max_iter, tol=tol)
    assert st == st_r and len(h) == len(rr)
    assert np.all(np.isfinite(x)) and np.array_equal(x, xr)
    assert _within_ulps(h, np.sqrt(rr), SQRT_ULPS), (h, np.sqrt(rr))


def test_invalid_arguments_write_nothing(ctx, oracle):
    import raptor_amd as ra

    O = oracle
    csr, Ao, b = _problem(O, B.GRIDS[1] + (0.5,))
    n = b.size
    ml = ra.ParMultilevel(**_options(O, "pmis+jacobi")[1]).setup(_local(ra, ctx, csr))
    x0 = O.vec_uniform(n, 5)
    dx, db = to_dev(ctx, x0), to_dev(ctx, b)
    with pytest.raises(ra.AmgError) as e:
        ml.bicgstab(dx, db, max_iter=-1)
    assert e.value.code == 1   # AMG_ERR_INVALID
    with pytest.raises(ra.AmgError) as e:
        ml.bicgstab(db, db, max_iter=3)   # x overlaps b
    assert e.value.code == 1
    assert np.array_equal(to_host(ctx, dx), x0) and np.array_equal(to_host(ctx, db), b)
    _, h, s = ml.bicgstab(dx, db, max_iter=2)   # the solver is still usable
    assert s == ra.AMG_KRYLOV_OK and len(h) == 3 and h[-1] < h[0]
