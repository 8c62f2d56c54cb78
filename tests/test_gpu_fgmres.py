"""Solver::fgmres (raptor_amd/csrc/multilevel.hip, the fgmres_* kernels of kernels.hip) against the
restatement of tests/fgmres_cases.py (checked on the CPU by tests/test_fgmres_cpu.py).

Bar: x and the whole history carry the restatement's bit patterns (compared as uint64) when the
restatement runs on the product's dot tree -- c, eta, the rotations, g and y all come from dot
products, so neither has an allowance -- on 1 rank and on 2 and 3 loopback ranks, with graphs on
and off, across restarts, at the dot spans' edges and in the exact cases."""
import ctypes as C

import numpy as np
import pytest

from tests import bicgstab_cases as B
from tests import cycle_option_cases as K
from tests import fgmres_cases as G
from tests.test_gpu_multirank import level_starts, run_ranks, set_oracle_cuts
from tests.util import loopback_ctx, to_dev, to_host

pytestmark = pytest.mark.gpu

GRID_IDS = ["x".join(map(str, d)) for d in B.GRIDS]
# (restart, max_iter): two full cycles plus one column; one open cycle (restart > max_iter);
# a cycle per iteration; max_iter an exact multiple of restart
RUNS = [(3, 7), (30, 6), (1, 4), (3, 6)]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(_bits(a), _bits(b)))


def _options(O, fam, **over):
    """(oracle options, product options) of a family, max_coarse = 32."""
    okw = K.oracle_options(O, fam, max_coarse=B.MAX_COARSE)
    pkw = K.product_options(fam, max_coarse=B.MAX_COARSE)
    pkw.update(over)
    return okw, pkw


def _local(ra, ctx, csr, lo=0, hi=None):
    """Rows [lo, hi) of a (row_ptr, col, val) matrix as a ParCSRMatrix."""
    rp, col, val = csr
    n = rp.size - 1
    hi = n if hi is None else hi
    return ra.ParCSRMatrix.from_csr(ctx, n, lo, rp[lo:hi + 1] - rp[lo], col[rp[lo]:rp[hi]],
                                    val[rp[lo]:rp[hi]])


_PROBLEMS = {}


def _problem(O, key):
    """key: (nx, ny, nz, pe) or ("chain", n, pe).  csr, oracle matrix, b."""
    if key not in _PROBLEMS:
        csr = G.operator(key)
        Ao = B.oracle_matrix(O, csr)
        b = B.rhs(O, Ao.shape[0])
        b.setflags(write=False)
        _PROBLEMS[key] = (csr, Ao, b)
    return _PROBLEMS[key]


_HIER = {}
_RESTATED = {}


def _hier(O, key, fam):
    if (key, fam) not in _HIER:
        _HIER[key, fam] = O.Hierarchy(_problem(O, key)[1], **_options(O, fam)[0])
    return _HIER[key, fam]


def _restated(O, key, fam, restart, max_iter, tol=0.0):
    """The one-rank restatement of a case from x = 0, computed once: x, hist, k, status."""
    k = (key, fam, restart, max_iter, tol)
    if k not in _RESTATED:
        _, Ao, b = _problem(O, key)
        out = G.fgmres_restated(_hier(O, key, fam), Ao, np.zeros(b.size), b, restart, max_iter, tol, K.dot_tree)
        out[0].setflags(write=False)
        _RESTATED[k] = out
    return _RESTATED[k]


def _zero(ctx, v):
    """v = 0 in place (the same device address), on the context's stream."""
    if getattr(ctx, "is_native", False):
        v.zero_()
        return
    import torch

    with torch.cuda.stream(ctx.stream):
        v.zero_()


# ---- 1. iterates ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", G.FAMS)
@pytest.mark.parametrize("pe", [0.0, 8.0])
@pytest.mark.parametrize("dims", B.GRIDS, ids=GRID_IDS)
def test_iterates_bit_exact(ctx, oracle, dims, pe, fam):
    """Every run of RUNS on one solver (fresh x each, so the restart changes between calls: 3 to
    30 regrows the workspace, 1 and 3 run in the larger one): x, the history, the count and the
    status are the restatement's."""
    import raptor_amd as ra

    O = oracle
    key = dims + (pe,)
    csr, Ao, b = _problem(O, key)
    ml = ra.ParMultilevel(**_options(O, fam)[1]).setup(_local(ra, ctx, csr))
    db = to_dev(ctx, b)
    for restart, max_iter in RUNS:
        xr, want, k, st_r = _restated(O, key, fam, restart, max_iter)
        assert st_r == G.KRYLOV_OK and k == max_iter and want.shape == (max_iter + 1,)
        dx = ctx.zeros(b.size)
        _, h, st = ml.fgmres(dx, db, max_iter=max_iter, restart=restart)
        assert st == ra.AMG_KRYLOV_OK, (restart, max_iter)
        assert _same(h, want), (restart, max_iter, h, want)
        assert _same(to_host(ctx, dx), xr), (restart, max_iter)


@pytest.mark.parametrize("fam", G.FAMS)
@pytest.mark.parametrize("pe", [0.0, 8.0])
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("dims", B.GRIDS, ids=GRID_IDS)
def test_iterates_bit_exact_ranks(oracle, dims, nranks, pe, fam):
    """Loopback ranks with ragged cuts: each rank's j + 1 dot values come from its own rows,
    travel in one allgather and are added in rank order."""
    import raptor_amd as ra

    O = oracle
    csr, Ao, b = _problem(O, dims + (pe,))
    n = b.size
    cuts = B.ragged_cuts(n, nranks)
    okw, pkw = _options(O, fam, replicate_below=0)
    Ho = O.Hierarchy(Ao, **okw)
    runs = RUNS[:3]

    def rank(r, nr, world):
        c = loopback_ctx(r, nr, world)
        lo, hi = cuts[r], cuts[r + 1]
        ml = ra.ParMultilevel(**pkw).setup(_local(ra, c, csr, lo, hi))
        db = to_dev(c, b[lo:hi])
        out = []
        for restart, max_iter in runs:
            dx = c.zeros(hi - lo)
            _, h, st = ml.fgmres(dx, db, max_iter=max_iter, restart=restart)
            out.append((to_host(c, dx), h, st))
        return out, level_starts(ml)

    res = run_ranks(nranks, rank)
    set_oracle_cuts(Ho, res)
    for q, (restart, max_iter) in enumerate(runs):
        xr, want, k, st_r = G.fgmres_restated(Ho, Ao, np.zeros(n), b, restart, max_iter, 0.0,
                                              lambda u, v: K.dot_tree(u, v, cuts))
        assert st_r == G.KRYLOV_OK and k == max_iter
        for r, (out, _) in enumerate(res):
            x, h, st = out[q]
            assert st == ra.AMG_KRYLOV_OK
            assert _same(h, want), (r, restart, h, want)
            assert _same(x, xr[cuts[r]:cuts[r + 1]]), (r, restart)


# ---- 2. stopping ----------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("restart", [5, 30])
@pytest.mark.parametrize("fam", G.FAMS)
@pytest.mark.parametrize("pe", [0.0, 8.0])
def test_tolerance_stops_at_the_restatements_iteration(ctx, oracle, pe, fam, restart, graph):
    """tol = 1e-8, cap 40 (the CPU module checks that no history ratio of these runs comes within
    1 % of the tolerance): the stop falls inside a cycle, and the closing launch applies exactly
    its completed columns: iterations, x and history are the restatement's."""
    import raptor_amd as ra

    O = oracle
    key = B.GRIDS[0] + (pe,)
    csr, Ao, b = _problem(O, key)
    xr, want, k, st_r = _restated(O, key, fam, restart, 40, 1e-8)
    assert st_r == G.KRYLOV_OK and 1 < k < 40
    ml = ra.ParMultilevel(**_options(O, fam, use_graph=graph)[1]).setup(_local(ra, ctx, csr))
    assert ml.graph_enabled == graph
    dx = ctx.zeros(b.size)
    _, h, st = ml.fgmres(dx, to_dev(ctx, b), max_iter=40, tol=1e-8, restart=restart)
    assert st == ra.AMG_KRYLOV_OK and len(h) == k + 1
    assert _same(h, want), (h, want)
    assert _same(to_host(ctx, dx), xr)
    assert h[-1] / h[0] < 1e-8 and np.all(h[:-1] / h[0] >= 1e-8)


# ---- 3. dot-span boundaries -----------------------------------------------------------------------
@pytest.mark.parametrize("pe", [0.5, 8.0])
@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_chain_sizes_on_the_dot_spans_edges(ctx, oracle, n, pe):
    """tridiag(-1 - pe, 2 + pe, -1), pmis + jacobi, restart 4, five iterations: one block to two
    blocks + 1 entry.  The multi-dot and update partials equal Solver::dot's there, or c, eta and
    with them every bit of x and the history would differ."""
    import raptor_amd as ra

    O = oracle
    key = ("chain", n, pe)
    csr, Ao, b = _problem(O, key)
    xr, want, k, st_r = _restated(O, key, "jacobi", 4, 5)
    assert st_r == G.KRYLOV_OK and k == 5 and np.all(np.isfinite(want))
    ml = ra.ParMultilevel(**_options(O, "jacobi")[1]).setup(_local(ra, ctx, csr))
    dx = ctx.zeros(n)
    _, h, st = ml.fgmres(dx, to_dev(ctx, b), max_iter=5, restart=4)
    assert st == ra.AMG_KRYLOV_OK
    assert _same(h, want), (h, want)
    assert _same(to_host(ctx, dx), xr)


# ---- 4. graphs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", G.FAMS)
def test_graphs_reuse_and_other_solvers_in_between(ctx, oracle, fam):
    """Graphs on and off give the same bits; a second call on the same solver and buffers replays
    the first call's graphs and equals a fresh solver's run; bicgstab and pcg between the two
    calls change nothing (and are not changed); a third call with a larger restart (workspace
    regrown, graphs dropped) matches the restatement."""
    import raptor_amd as ra

    O = oracle
    key = B.GRIDS[0] + (8.0,)
    csr, Ao, b = _problem(O, key)
    n = b.size
    xr, want, _, _ = _restated(O, key, fam, 3, 7)
    xr2, want2, _, _ = _restated(O, key, fam, 9, 11)
    A = _local(ra, ctx, csr)
    for graph in (True, False):
        pkw = _options(O, fam, use_graph=graph)[1]
        ml = ra.ParMultilevel(**pkw).setup(A)
        assert ml.graph_enabled == graph
        dx, db = ctx.zeros(n), to_dev(ctx, b)
        dp, dq = ctx.zeros(n), ctx.zeros(n)
        for call in range(2):
            if call:
                _zero(ctx, dx)
            _, h, st = ml.fgmres(dx, db, max_iter=7, restart=3)
            assert st == ra.AMG_KRYLOV_OK
            assert _same(h, want), (graph, call)
            assert _same(to_host(ctx, dx), xr), (graph, call)
            if call == 0:
                ml.bicgstab(dp, db, max_iter=3)   # their own graph slots and buffers
                ml.pcg(dq, db, max_iter=3)
        _zero(ctx, dx)
        _, h, st = ml.fgmres(dx, db, max_iter=11, restart=9)
        assert st == ra.AMG_KRYLOV_OK
        assert _same(h, want2), graph
        assert _same(to_host(ctx, dx), xr2), graph
        fresh = ra.ParMultilevel(**pkw).setup(A)
        fp, fq, fx = ctx.zeros(n), ctx.zeros(n), ctx.zeros(n)
        fresh.bicgstab(fp, db, max_iter=3)
        fresh.pcg(fq, db, max_iter=3)
        assert _same(to_host(ctx, dp), to_host(ctx, fp))   # unchanged by fgmres
        assert _same(to_host(ctx, dq), to_host(ctx, fq))
        _, hf, _ = fresh.fgmres(fx, db, max_iter=7, restart=3)
        assert _same(hf, want) and _same(to_host(ctx, fx), xr)


# ---- 5. exact and one-level cases -----------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("tol", [0.0, 1e-8])
def test_one_by_one_is_a_happy_breakdown(ctx, oracle, tol, graph):
    """n = 1, A = [4], b = [3]: eta == 0 exactly in the first column: one iteration, hist =
    [3, 0], x = 0.75, status OK; with tol = 0 the three replays after the stop change nothing."""
    import raptor_amd as ra

    O = oracle
    one = np.array([0, 1], np.int64), np.array([0], np.int64), np.array([4.0])
    ml = ra.ParMultilevel(**_options(O, "jacobi", use_graph=graph)[1]).setup(_local(ra, ctx, one))
    dx = ctx.zeros(1)
    _, h, st = ml.fgmres(dx, to_dev(ctx, np.array([3.0])), max_iter=4, tol=tol, restart=5)
    assert st == ra.AMG_KRYLOV_OK and _same(h, np.array([3.0, 0.0]))
    assert _same(to_host(ctx, dx), np.array([0.75]))


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("tol", [0.0, 1e-8])
def test_exact_start_and_zero_limit_leave_x(ctx, oracle, tol, graph):
    """b = A x0 by the product's own mult: r is exactly 0: no iteration, hist = [0], status OK, x
    untouched (with tol = 0 the ten gated replays change nothing).  max_iter = 0 on another b:
    hist = [beta], x untouched."""
    import raptor_amd as ra

    O = oracle
    csr, Ao, b = _problem(O, B.GRIDS[1] + (0.5,))
    n = Ao.shape[0]
    A = _local(ra, ctx, csr)
    ml = ra.ParMultilevel(**_options(O, "jacobi", use_graph=graph)[1]).setup(A)
    x0 = np.rint(8 * O.vec_uniform(n, 3))
    dx, db = to_dev(ctx, x0), ctx.zeros(n)
    A.mult(dx, db)
    assert not np.any(Ao.residual(x0, to_host(ctx, db)))
    _, h, st = ml.fgmres(dx, db, max_iter=10, tol=tol, restart=4)
    assert st == ra.AMG_KRYLOV_OK and h.tolist() == [0.0]
    assert _same(to_host(ctx, dx), x0)
    _, h, st = ml.fgmres(dx, to_dev(ctx, b), max_iter=0, tol=tol, restart=4)
    r = Ao.residual(x0, b)
    assert st == ra.AMG_KRYLOV_OK and _same(h, np.array([np.sqrt(K.dot_tree(r, r))]))
    assert _same(to_host(ctx, dx), x0)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_one_level_run_against_the_restatement(ctx, oracle, graph):
    """A 24-row chain under max_coarse = 32: M is the coarse solve, so after the first column eta
    is of the order 1e-16 and the later columns orthogonalise noise -- six iterations at restart 3
    with tol = 0 still carry the restatement's bits."""
    import raptor_amd as ra

    O = oracle
    key = ("chain", 24, 2.0)
    csr, Ao, b = _problem(O, key)
    assert _hier(O, key, "jacobi").num_levels == 1
    xr, want, k, st_r = _restated(O, key, "jacobi", 3, 6)
    ml = ra.ParMultilevel(**_options(O, "jacobi", use_graph=graph)[1]).setup(_local(ra, ctx, csr))
    dx = ctx.zeros(24)
    _, h, st = ml.fgmres(dx, to_dev(ctx, b), max_iter=6, restart=3)
    assert st == st_r and len(h) == k + 1
    assert _same(h, want), (h, want)
    assert np.all(np.isfinite(xr)) and _same(to_host(ctx, dx), xr)


# ---- 6. the symmetric case ------------------------------------------------------------------------
def test_symmetric_operator_converges_like_pcg(ctx, oracle):
    """pe = 0 is the symmetric 7-point operator: pcg and fgmres both reach 1e-8 (FGMRES is not
    held to PCG's count), and both true residuals confirm it."""
    import raptor_amd as ra

    O = oracle
    csr, Ao, b = _problem(O, B.GRIDS[0] + (0.0,))
    n = b.size
    ml = ra.ParMultilevel(**_options(O, "jacobi")[1]).setup(_local(ra, ctx, csr))
    db = to_dev(ctx, b)
    dp, dx = ctx.zeros(n), ctx.zeros(n)
    _, hp = ml.pcg(dp, db, max_iter=40, tol=1e-8)
    _, h, st = ml.fgmres(dx, db, max_iter=40, tol=1e-8)
    assert st == ra.AMG_KRYLOV_OK
    assert len(hp) <= 40 and len(h) <= 40 and hp[-1] / hp[0] < 1e-8 and h[-1] / h[0] < 1e-8
    b0 = O.norm2(b)
    assert O.norm2(Ao.residual(to_host(ctx, dp), b)) < 2e-8 * b0
    assert O.norm2(Ao.residual(to_host(ctx, dx), b)) < 2e-8 * b0


# ---- 7. contract ----------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(ctx, oracle):
    """restart 0 and 65, max_iter -1, x overlapping b: AMG_ERR_INVALID, and x, b, the history
    with a guard band on either side, *iters and *status keep their bits."""
    import raptor_amd as ra

    O = oracle
    csr, Ao, b = _problem(O, B.GRIDS[1] + (0.5,))
    n = b.size
    ml = ra.ParMultilevel(**_options(O, "jacobi")[1]).setup(_local(ra, ctx, csr))
    x0 = O.vec_uniform(n, 5)
    dx, db = to_dev(ctx, x0), to_dev(ctx, b)
    guard, cap = 16, 8
    hist0 = O.vec_uniform(cap + 1 + 2 * guard, 9)
    hist = hist0.copy()
    hp = C.cast(hist.ctypes.data + 8 * guard, C.POINTER(C.c_double))
    L = ra.lib()
    for x, restart, max_iter in [(dx, 0, 3), (dx, G.MAX_RESTART + 1, 3), (dx, -1, 3), (dx, 3, -1), (db, 3, 3)]:
        it, st = C.c_int32(-7), C.c_int32(-9)
        rc = L.amg_solver_fgmres(ml.h, ra._ptr(x), ra._ptr(db), restart, max_iter, 0.0, hp,
                                 C.byref(it), C.byref(st))
        assert rc == 1, (restart, max_iter)   # AMG_ERR_INVALID
        assert (it.value, st.value) == (-7, -9)
        assert _same(hist, hist0)
        assert _same(to_host(ctx, dx), x0) and _same(to_host(ctx, db), b)
    with pytest.raises(ra.AmgError) as e:
        ml.fgmres(dx, db, max_iter=3, restart=0)
    assert e.value.code == 1
    _, h, s = ml.fgmres(dx, db, max_iter=2, restart=G.MAX_RESTART)   # the solver is still usable
    assert s == ra.AMG_KRYLOV_OK and len(h) == 3 and h[-1] < h[0]
