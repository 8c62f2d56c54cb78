"""The solve layer on the GPU (Solver::cycle_rec, smooth, solve, pcg, dot and the graph slots in
raptor_amd/csrc/multilevel.hip) under every cycle option, against the CPU oracle and the
restatements of tests/cycle_option_cases.py (checked on the CPU by test_cycle_options_cpu.py).

Bars: V-cycle and solve iterates bit-identical to the oracle's for every (pre, post, omega,
gs_block); PCG iterates bit-identical to the oracle's loop run on the product's dot tree (alpha
and beta come from r.z and p.q, so x has no allowance); PCG history entries within SQRT_ULPS of
np.sqrt(rr_k), for the device sqrt of finish_sum_kernel -- equal in the one-rank chain test,
where all 220 entries came out equal on the MI355X; solve histories within 1e-10 relative, fused
norms within 1e-12."""
import numpy as np
import pytest

from tests import cycle_option_cases as K
from tests.test_gpu_multirank import level_starts, run_ranks, set_oracle_cuts
from tests.util import loopback_ctx, same_csr, to_dev, to_host

pytestmark = pytest.mark.gpu

# allowance on a PCG history entry against np.sqrt of the restated squared norm: the rounding of
# the device sqrt in finish_sum_kernel (dropped where the entries were seen to be equal)
SQRT_ULPS = 2


def _frozen(a):
    a = np.array(a, np.float64)
    a.setflags(write=False)
    return a


def _setenv(monkeypatch, env):
    for k, v in K.ENVS[env].items():
        monkeypatch.setenv(k, v)


def _same_hierarchy(ml, mats):
    assert ml.num_levels == len(mats)
    for l, (A, P, R) in enumerate(mats):
        assert same_csr(ml.level_matrix(l, "A").to_scipy_local(), A), ("A", l)
        if l + 1 < len(mats):
            assert same_csr(ml.level_matrix(l, "P").to_scipy_local(), P), ("P", l)
            assert same_csr(ml.level_matrix(l, "R").to_scipy_local(), R), ("R", l)


def _oracle_mats(Ho):
    return [(Ho.matrix(l, "A"), Ho.matrix(l, "P"), Ho.matrix(l, "R")) for l in range(Ho.num_levels)]


def _hist_close(h, ho, rel):
    return h.shape == ho.shape and bool(np.all(np.abs(h - ho) <= rel * ho))


def _within_ulps(h, want, ulps):
    return h.shape == want.shape and bool(np.all(np.abs(h - want) <= ulps * np.spacing(want)))


def _zero(ctx, v):
    """v = 0 in place (the same device address), on the context's stream."""
    if getattr(ctx, "is_native", False):
        v.zero_()
    else:
        import torch

        with torch.cuda.stream(ctx.stream):
            v.zero_()
    return v


# ---- 3. the option matrix --------------------------------------------------------------------
_REFS = {}


def _option_ref(O, kind, fam, pre, post, w, B):
    """The oracle's side of an option case, computed once and shared by the builds (envs)."""
    key = (kind, fam, pre, post, w, B)
    if key not in _REFS:
        Ao, b = K.problem(O, kind)
        Ho = O.Hierarchy(Ao, **K.oracle_options(O, fam, pre, post, w, B))
        n = b.size
        xs, x = [], np.zeros(n)
        for _ in range(4):
            x = Ho.cycle(x, b)
            xs.append(_frozen(x))
        sx, sh = Ho.solve(np.zeros(n), b, max_iter=6)
        _REFS[key] = dict(b=_frozen(b), mats=_oracle_mats(Ho), cycles=xs, solve_x=_frozen(sx),
                          solve_hist=_frozen(sh))
    return _REFS[key]


def _bytes_model(ml, l, pre, post, jacobi):
    """Solver::bytes_per_cycle restated: plain-CSR bytes of level l's share of one V-cycle
    (12 B per entry + row_ptr; a sweep moves b, x, dinv in and x out)."""
    inf = ml.level_info(l)
    n, nnz = inf["n_local"], inf["nnz_local"]
    if l + 1 == ml.num_levels:
        cn = inf["n_global"]
        return 8 * cn * n + 8 * cn + 8 * n
    nc = ml.level_info(l + 1)["n_local"]
    base = 12 * nnz + 4 * (n + 1)
    sweep = base + 32 * n
    total, zero = 0, l > 0
    for _ in range(pre):
        if zero and jacobi:
            total += 24 * n                      # omega dinv b
        else:
            total += sweep + (8 * n if zero else 0)  # (zero fill of x first)
        zero = False
    if zero:
        total += 8 * n                           # no pre-sweep: x zeroed by itself
    total += base + 24 * n                                              # residual
    total += 12 * inf["r_nnz_local"] + 4 * (nc + 1) + 8 * n + 8 * nc    # restriction
    total += 12 * inf["p_nnz_local"] + 4 * (n + 1) + 8 * nc + 8 * n + 8 * n  # interpolation
    total += post * sweep
    if (pre + post) % 2 == 1:
        total += 16 * n                          # copy back
    return total


@pytest.mark.parametrize("case", K.gpu_matrix(), ids=K.case_id)
def test_cycle_options_bit_exact(ctx, oracle, monkeypatch, case):
    """Every (pre, post, omega / gs_block): the hierarchy is the oracle's, four V-cycles from
    x = 0 and a 6-cycle solve are the oracle's bit for bit, replayed from graphs and launched
    eagerly; the byte model follows the sweep counts."""
    import raptor_amd as ra

    kind, env, fam, pre, post, w, B = case
    _setenv(monkeypatch, env)
    ref = _option_ref(oracle, kind, fam, pre, post, w, B)
    A = ra.par_stencil_grid(ctx, kind, K.PROBLEMS[kind])
    n = A.local_rows
    db = to_dev(ctx, ref["b"])
    for graph in (True, False):
        ml = ra.ParMultilevel(use_graph=graph, **K.product_options(fam, pre, post, w, B)).setup(A)
        assert ml.graph_enabled == graph
        if graph:
            assert ml.num_levels >= 4
            _same_hierarchy(ml, ref["mats"])
            for l in range(ml.num_levels):
                assert ml.level_info(l)["bytes_per_cycle_local"] == \
                    _bytes_model(ml, l, pre, post, fam == "jacobi"), ("bytes", l)
            if env == "tpl":
                assert A.info["template_rows"] > 0
            if env == "split":
                split = [ml.level_matrix(l, "A").info["gs_split"] for l in range(ml.num_levels - 1)]
                assert all(split), split
        dx = ctx.zeros(n)
        for k in range(4):
            ml.cycle(dx, db)
            assert np.array_equal(to_host(ctx, dx), ref["cycles"][k]), ("cycle", k, graph)
        dx = ctx.zeros(n)
        _, hist = ml.solve(dx, db, max_iter=6)
        assert np.array_equal(to_host(ctx, dx), ref["solve_x"]), ("solve", graph)
        assert _hist_close(hist, ref["solve_hist"], 1e-10), (graph, hist, ref["solve_hist"])
        if pre >= 1:  # every entry but the last left by a cycle's first sweep (fused norm)
            assert _hist_close(hist, ref["solve_hist"], 1e-12), (graph, hist, ref["solve_hist"])


@pytest.mark.parametrize("rep", [0, 10 ** 9], ids=["distributed", "rep-all"])
@pytest.mark.parametrize("pre,post", [(0, 1), (2, 2)])
@pytest.mark.parametrize("fam", list(K.FAMILIES))
@pytest.mark.parametrize("nranks", [2, 3])
def test_cycle_options_multirank(oracle, nranks, fam, pre, post, rep):
    """Loopback ranks: every rank's slice of three V-cycles is the oracle's (hybrid GS with the
    oracle's blocks cut at the ranks' rows), levels distributed or replicated below level 0."""
    import raptor_amd as ra

    O = oracle
    kind = "7pt"
    w, B = (1.0, 8) if (pre, post) == (0, 1) else (0.5, 64)
    Ao, b = K.problem(O, kind)
    Ho = O.Hierarchy(Ao, **K.oracle_options(O, fam, pre, post, w, B))
    n = b.size

    def rank(r, nr, world):
        c = loopback_ctx(r, nr, world)
        A = ra.par_stencil_grid(c, kind, K.PROBLEMS[kind])
        ml = ra.ParMultilevel(replicate_below=rep, **K.product_options(fam, pre, post, w, B)).setup(A)
        f, m = A.first_row, A.local_rows
        dx, db = c.zeros(m), to_dev(c, b[f:f + m])
        xs = []
        for _ in range(3):
            ml.cycle(dx, db)
            xs.append(to_host(c, dx))
        return ml.num_levels, f, m, xs, level_starts(ml)

    res = run_ranks(nranks, rank)
    assert sum(m for _, _, m, _, _ in res) == n
    set_oracle_cuts(Ho, res)
    xo = np.zeros(n)
    for k in range(3):
        xo = Ho.cycle(xo, b)
        for nl, f, m, xs, _ in res:
            assert nl == Ho.num_levels >= 4
            assert np.array_equal(xs[k], xo[f:f + m]), ("cycle", k, f)


# ---- 4. stopping rules and state across calls -------------------------------------------------
_STOP_REFS = {}


def _stop_problem(O, fam):
    """7-pt problem, default options (max_coarse as in the matrix): matrix, b, oracle hierarchy."""
    if fam not in _STOP_REFS:
        Ao, b = K.problem(O, "7pt")
        _STOP_REFS[fam] = (Ao, _frozen(b), O.Hierarchy(Ao, **K.oracle_options(O, fam)))
    return _STOP_REFS[fam]


def _stop_solver(ra, ctx, fam, graph=None):
    A = ra.par_stencil_grid(ctx, "7pt", K.PROBLEMS["7pt"])
    return A, ra.ParMultilevel(use_graph=graph, **K.product_options(fam)).setup(A)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("fam,what", list(K.STOP))
def test_tolerance_stops_at_the_oracles_iteration(ctx, oracle, fam, what, graph):
    """solve / pcg with a tolerance stop at the oracle's iteration (the CPU module checks that
    no history ratio comes within 1 % of the tolerance) with the reference's iterate."""
    import raptor_amd as ra

    Ao, b, Ho = _stop_problem(oracle, fam)
    n = b.size
    kw = K.STOP[fam, what]
    A, ml = _stop_solver(ra, ctx, fam, graph)
    dx, db = ctx.zeros(n), to_dev(ctx, b)
    if what == "solve":
        xo, ho = Ho.solve(np.zeros(n), b, **kw)
        _, h = ml.solve(dx, db, **kw)
        assert len(h) == len(ho) and 1 < len(h) <= kw["max_iter"]
        assert np.array_equal(to_host(ctx, dx), xo)
        assert _hist_close(h, ho, 1e-10)
    else:
        _, ho = Ho.pcg(np.zeros(n), b, **kw)
        xr, rr = K.pcg_restated(Ho, Ao, np.zeros(n), b, kw["max_iter"], kw["tol"], K.dot_tree)
        _, h = ml.pcg(dx, db, **kw)
        assert len(h) == len(ho) == len(rr) and 1 < len(h) <= kw["max_iter"]
        assert np.array_equal(to_host(ctx, dx), xr)
        assert _within_ulps(h, np.sqrt(rr), SQRT_ULPS), (h, np.sqrt(rr))
    assert h[-1] / h[0] < kw["tol"] and np.all(h[:-1] / h[0] >= kw["tol"])


@pytest.mark.parametrize("fam", list(K.FAMILIES))
def test_unfused_loop_equals_fused_loop(ctx, oracle, fam):
    """tol = 1e-300 never stops but takes the loop with a stand-alone residual pass per cycle;
    tol = 0 takes the norms from each cycle's first sweep.  Same iterates, bit for bit, and the
    last history entry -- the stand-alone pass in both -- is equal."""
    import raptor_amd as ra

    Ao, b, Ho = _stop_problem(oracle, fam)
    n = b.size
    for graph in (True, False):
        A, ml = _stop_solver(ra, ctx, fam, graph)
        db = to_dev(ctx, b)
        for iters in (1, 2, 4):
            xo, ho = Ho.solve(np.zeros(n), b, max_iter=iters)
            got = []
            for tol in (0.0, 1e-300):
                dx = ctx.zeros(n)
                _, h = ml.solve(dx, db, max_iter=iters, tol=tol)
                got.append((to_host(ctx, dx), h))
            (xf, hf), (xu, hu) = got
            assert np.array_equal(xf, xo) and np.array_equal(xu, xo), (graph, iters)
            assert hf.shape == hu.shape == (iters + 1,)
            assert hf[-1] == hu[-1], (graph, iters)
            assert _hist_close(hf, ho, 1e-12) and _hist_close(hu, ho, 1e-12)


@pytest.mark.parametrize("fam", list(K.FAMILIES))
def test_zero_iterations_and_zero_rhs(ctx, oracle, fam):
    """max_iter = 0: x untouched, hist = [||b - A x||] (solve and pcg).  b = 0 from x = 0: the
    history is all 0.0 and x stays 0.0 (solve divides by nothing on this path)."""
    import raptor_amd as ra

    O = oracle
    Ao, b, Ho = _stop_problem(O, fam)
    n = b.size
    A, ml = _stop_solver(ra, ctx, fam)
    x0 = O.vec_uniform(n, 5)
    r = Ao.residual(x0, b)
    db = to_dev(ctx, b)
    for tol in (0.0, 1e-3):
        dx = to_dev(ctx, x0)
        _, h = ml.solve(dx, db, max_iter=0, tol=tol)
        assert np.array_equal(to_host(ctx, dx), x0)
        assert h.shape == (1,) and abs(h[0] - O.norm2(r)) <= 1e-12 * O.norm2(r)
        dx = to_dev(ctx, x0)
        _, h = ml.pcg(dx, db, max_iter=0, tol=tol)
        assert np.array_equal(to_host(ctx, dx), x0)
        assert _within_ulps(h, np.sqrt(np.array([K.dot_tree(r, r)])), SQRT_ULPS)
    dz = ctx.zeros(n)
    for tol in (0.0, 1e-6):
        dx = ctx.zeros(n)
        _, h = ml.solve(dx, dz, max_iter=3, tol=tol)
        assert h.tolist() == [0.0] * 4, (tol, h)
        assert not np.any(to_host(ctx, dx))
    assert not np.any(to_host(ctx, dz))


@pytest.mark.parametrize("fam", list(K.FAMILIES))
def test_one_solver_through_many_calls(ctx, oracle, fam):
    """Graphs are keyed by the (x, b) addresses, dropped when the history buffer grows past
    1024 entries or PCG's scratch is first allocated, and can be switched off and on: whatever
    a live solver went through, each call gives what a fresh solver gives, bit for bit."""
    import raptor_amd as ra

    O = oracle
    _, b1, _ = _stop_problem(O, fam)
    n = b1.size
    b2 = O.vec_uniform(n, 7)
    A, ml = _stop_solver(ra, ctx, fam)
    assert ml.graph_enabled
    dev = {"b1": to_dev(ctx, b1), "b2": to_dev(ctx, b2),
           "x1": ctx.zeros(n), "x2": ctx.zeros(n), "x3": ctx.zeros(n)}
    host_b = {"b1": b1, "b2": b2}
    # (method, x, b, arguments, graphs for this and later calls or None, zero x first)
    calls = [("solve", "x1", "b1", dict(max_iter=3), None, False),
             ("solve", "x2", "b2", dict(max_iter=3), None, False),
             ("solve", "x1", "b1", dict(max_iter=3), None, True),
             ("pcg", "x1", "b1", dict(max_iter=5), None, False),
             ("solve", "x3", "b1", dict(max_iter=1100, tol=1e-6), None, False),
             ("solve", "x2", "b2", dict(max_iter=3), False, False),
             ("solve", "x1", "b1", dict(max_iter=3), True, False),
             ("pcg", "x2", "b2", dict(max_iter=5), None, False)]
    graph = True
    for step, (what, xk, bk, kw, set_graph, zero) in enumerate(calls):
        if set_graph is not None:
            ml.set_graph(set_graph)
            graph = set_graph
        assert ml.graph_enabled == graph
        if zero:
            _zero(ctx, dev[xk])
        before = to_host(ctx, dev[xk])
        _, h = getattr(ml, what)(dev[xk], dev[bk], **kw)
        after = to_host(ctx, dev[xk])
        _, fresh = _stop_solver(ra, ctx, fam, graph)
        fx = to_dev(ctx, before)
        _, fh = getattr(fresh, what)(fx, to_dev(ctx, host_b[bk]), **kw)
        assert np.array_equal(after, to_host(ctx, fx)), (step, what)
        assert np.array_equal(h, fh), (step, what, h, fh)
        if "tol" in kw:
            assert 1 < len(h) < 100 and h[-1] / h[0] < kw["tol"]
        else:
            assert len(h) == kw["max_iter"] + 1
        assert np.all(np.isfinite(h)) and h[-1] < h[0]


def test_bad_options_raise_and_leave_the_context_usable(ctx, oracle):
    import raptor_amd as ra

    O = oracle
    Ao, b, Ho = _stop_problem(O, "gs")
    A = ra.par_stencil_grid(ctx, "7pt", K.PROBLEMS["7pt"])
    bad = [dict(K.product_options("gs"), gs_block=0), dict(K.product_options("gs"), gs_block=65),
           dict(K.product_options("gs"), max_levels=0), dict(K.product_options("jacobi"), max_levels=0),
           dict(K.product_options("jacobi"), pre_sweeps=-1), dict(K.product_options("gs"), post_sweeps=-1)]
    for kw in bad:
        with pytest.raises(ra.AmgError):
            ra.ParMultilevel(**kw).setup(A)
    ml = ra.ParMultilevel(**K.product_options("gs")).setup(A)
    dx = ctx.zeros(b.size)
    ml.cycle(dx, to_dev(ctx, b))
    assert np.array_equal(to_host(ctx, dx), Ho.cycle(np.zeros(b.size), b))


# ---- 5. PCG and its reductions ----------------------------------------------------------------
def _chain_oracle(O, fam, n):
    Ao, b, csr = K.chain_problem(O, n)
    Ho = O.Hierarchy(Ao, **K.oracle_options(O, fam, max_coarse=K.CHAIN_MAX_COARSE))
    return Ao, b, csr, Ho


@pytest.mark.parametrize("fam", list(K.FAMILIES))
@pytest.mark.parametrize("n", K.CHAIN_SIZES)
def test_pcg_bit_exact_on_the_dot_tree(ctx, oracle, n, fam):
    """1-D chain, sizes on the dot span's edges: ten PCG iterations give the x of the oracle's
    loop run on the restated dot tree, graphs on and off; the history is sqrt(rr_k)."""
    import raptor_amd as ra

    O = oracle
    Ao, b, (rp, col, val), Ho = _chain_oracle(O, fam, n)
    xr, rr = K.pcg_restated(Ho, Ao, np.zeros(n), b, 10, 0.0, K.dot_tree)
    want = np.sqrt(rr)
    assert want.shape == (11,) and np.all(want > 0)
    A = ra.ParCSRMatrix.from_csr(ctx, n, 0, rp, col, val)
    db = to_dev(ctx, b)
    for graph in (True, False):
        ml = ra.ParMultilevel(use_graph=graph,
                              **K.product_options(fam, max_coarse=K.CHAIN_MAX_COARSE)).setup(A)
        if graph:
            _same_hierarchy(ml, _oracle_mats(Ho))
        dx = ctx.zeros(n)
        _, h = ml.pcg(dx, db, max_iter=10)
        assert np.array_equal(to_host(ctx, dx), xr), graph
        assert np.array_equal(h, want), (graph, h, want)


@pytest.mark.parametrize("fam", list(K.FAMILIES))
def test_pcg_bit_exact_three_ranks(oracle, fam):
    """The chain cut at rows [0, 2049, 2050, 4097] (one span + 1 | one row | 2047 rows): each
    rank's dot value comes from its own slice and the values are added in rank order."""
    import raptor_amd as ra

    O = oracle
    n = K.CHAIN_CUTS[-1]
    cuts = K.CHAIN_CUTS
    Ao, b, (rp, col, val), Ho = _chain_oracle(O, fam, n)

    def rank(r, nr, world):
        c = loopback_ctx(r, nr, world)
        lo, hi = cuts[r], cuts[r + 1]
        A = ra.ParCSRMatrix.from_csr(c, n, lo, rp[lo:hi + 1] - rp[lo], col[rp[lo]:rp[hi]],
                                     val[rp[lo]:rp[hi]])
        ml = ra.ParMultilevel(replicate_below=0,
                              **K.product_options(fam, max_coarse=K.CHAIN_MAX_COARSE)).setup(A)
        dx = c.zeros(hi - lo)
        _, h = ml.pcg(dx, to_dev(c, b[lo:hi]), max_iter=10)
        return ml.num_levels, to_host(c, dx), h, level_starts(ml)

    res = run_ranks(3, rank)
    set_oracle_cuts(Ho, res)
    xr, rr = K.pcg_restated(Ho, Ao, np.zeros(n), b, 10, 0.0, lambda u, v: K.dot_tree(u, v, cuts))
    want = np.sqrt(rr)
    for r, (nl, x, h, _) in enumerate(res):
        assert nl == Ho.num_levels
        assert np.array_equal(x, xr[cuts[r]:cuts[r + 1]]), r
        assert _within_ulps(h, want, SQRT_ULPS), (r, h, want)
        assert np.array_equal(h, res[0][2])  # every rank reports the same history


def test_norm_reduction_over_two_blocks(ctx, oracle):
    """7-pt 66 x 64 x 64 in the blocks format leaves more than 4096 norm partials, so
    reduce_norm_kernel runs two blocks and the last one to arrive sums their sums and resets
    the arrival counter: the solver's norm equals the two-launch reduction's bit for bit, is the
    oracle's within 1e-12, and stays the same over 20 calls."""
    import raptor_amd as ra

    O = oracle
    dims = (66, 64, 64)
    Ao = O.gen_7pt(*dims)
    n = Ao.shape[0]
    A = ra.par_stencil_grid(ctx, "7pt", dims).set_format("blocks")
    x0, b = O.vec_uniform(n, 3), Ao.spmv(O.vec_uniform(n, 42))
    dx, db = to_dev(ctx, x0), to_dev(ctx, b)
    two_launch = A.residual_norm(dx, db)
    assert 4 * A.info["n_blocks"] > 4096
    want = O.norm2(Ao.residual(x0, b))
    assert abs(two_launch - want) <= 1e-12 * want
    ml = ra.ParMultilevel().setup(A)
    assert 4 * ml.level_matrix(0, "A").info["n_blocks"] > 4096
    for graph in (True, False):
        ml.set_graph(graph)
        for _ in range(10):
            _, h = ml.solve(dx, db, max_iter=0)
            assert h.tolist() == [two_launch]
    Ho = O.Hierarchy(Ao, **O.DEFAULTS["pmis"])
    xo, ho = Ho.solve(np.zeros(n), b, max_iter=3)
    for graph in (True, False):
        ml.set_graph(graph)
        dx = ctx.zeros(n)
        _, h = ml.solve(dx, db, max_iter=3)
        assert np.array_equal(to_host(ctx, dx), xo)
        assert _hist_close(h, ho, 1e-12), (h, ho)
