"""Multicolour Gauss-Seidel on the GPU (colour_rows in setup_device.hip, mc_gs.hip, Solver::smooth
in multilevel.hip) against the restatement of tests/mc_gs_cases.py (checked on the CPU by
tests/test_mc_gs_cpu.py).

Bars: colours and readiness rounds equal the restatement's on 1, 2 and 3 loopback ranks; sweeps
(forward, backward; a launch per colour, one workgroup, automatic) bit-identical to the
restatement, to int64 arithmetic on integer operands and at fixed points; rows a poisoned column
cannot reach keep the restated bits; V-cycles, solve, PCG and BiCGStab iterates bit-identical to
the scaffold on 1, 2 and 3 ranks; solve histories within 1e-10 relative, Krylov histories within
SQRT_ULPS of sqrt(rr_k) (tests/test_gpu_cycle_options.py).  Small shapes only."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import bicgstab_cases as B
from tests import cycle_option_cases as K
from tests import edge_cases as E
from tests import mc_gs_cases as M
from tests.edge_cases import bits
from tests.test_gpu_cycle_options import SQRT_ULPS
from tests.test_gpu_multirank import run_ranks
from tests.util import loopback_ctx, same_csr, to_dev, to_host

pytestmark = pytest.mark.gpu

PATHS = {"auto": 0, "per-colour": 1, "one-workgroup": 2}


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


def _diff(a, b):
    return np.flatnonzero(bits(a) != bits(b))


def _frozen(a):
    a = np.array(a, np.float64)
    a.setflags(write=False)
    return a


def _up(ctx, a):
    return to_dev(ctx, np.array(a, np.float64))  # a writable copy (the references are frozen)


def _dev(ra, ctx, A, lo=0, hi=None):
    """Rows [lo, hi) of a scipy CSR as a ParCSRMatrix (explicit zeros kept)."""
    n = A.shape[0]
    hi = n if hi is None else hi
    rp = A.indptr
    return ra.ParCSRMatrix.from_csr(ctx, n, lo, rp[lo:hi + 1] - rp[lo], A.indices[rp[lo]:rp[hi]],
                                    A.data[rp[lo]:rp[hi]])


_OPS, _REFS = {}, {}


def _ops(O):
    if not _OPS:
        _OPS.update(M.operators(O))
    return _OPS


def _ref(O, name):
    """Per operator, once: colours, rounds, and the restated sweeps of vec_uniform data."""
    if name not in _REFS:
        A = _ops(O)[name]
        Ao = O.Csr.from_scipy(A)
        n = A.shape[0]
        c, r = M.first_fit(A, M.SEED)
        x, b = O.vec_uniform(n, 3), O.vec_uniform(n, 4)
        ref = dict(A=A, Ao=Ao, colour=c, rounds=r, x=x, b=b, fwd=M.sweep(Ao, c, x, b, False),
                   bwd=M.sweep(Ao, c, x, b, True), b_fixed=Ao.spmv(x))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[name] = ref
    return _REFS[name]


def _sweep(ctx, A, x, b, backward, path):
    dx = _up(ctx, x)
    A.mc_gs(dx, _up(ctx, b), backward=backward, path=path)
    return to_host(ctx, dx)


# ---- 1. the colouring ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.OPERATORS)
def test_colours_one_rank(ctx, oracle, name):
    import raptor_amd as ra

    ref = _ref(oracle, name)
    A = _dev(ra, ctx, ref["A"])
    assert A.info["mc_gs_bytes"] == 0
    nc = A.colour(M.SEED)
    got = A.colours()
    assert np.array_equal(got, ref["colour"]), np.flatnonzero(got != ref["colour"])[:8]
    assert nc == ref["colour"].max() + 1 and A.colour_rounds() == ref["rounds"]
    assert A.info["mc_gs_bytes"] > 12 * ref["A"].nnz
    # another seed: another order, the restatement's again
    other, _ = M.first_fit(ref["A"], M.SEED + 1)
    assert A.colour(M.SEED + 1) == other.max() + 1 and np.array_equal(A.colours(), other)


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("name", M.OPERATORS)
def test_colours_loopback_ranks(oracle, name, nranks):
    import raptor_amd as ra

    ref = _ref(oracle, name)
    Asp = ref["A"]
    cuts = M.cuts(Asp.shape[0], nranks)

    def rank(r, nr, world):
        c = loopback_ctx(r, nr, world)
        A = _dev(ra, c, Asp, cuts[r], cuts[r + 1])
        return A.colour(M.SEED), A.colours(), A.colour_rounds()

    for r, (nc, got, rounds) in enumerate(run_ranks(nranks, rank)):
        assert np.array_equal(got, ref["colour"][cuts[r]:cuts[r + 1]]), r
        assert nc == ref["colour"].max() + 1 and rounds == ref["rounds"]


# ---- 2. the sweep ----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", M.OPERATORS)
def test_sweep_bit_exact(ctx, oracle, name, path):
    """Forward and backward against the restatement; with b = A x the sweep returns x itself; the
    three paths give the same bits (each equals the restatement)."""
    import raptor_amd as ra

    ref = _ref(oracle, name)
    A = _dev(ra, ctx, ref["A"])
    A.colour(M.SEED)
    p = PATHS[path]
    for back, want in ((False, ref["fwd"]), (True, ref["bwd"])):
        got = _sweep(ctx, A, ref["x"], ref["b"], back, p)
        assert _same(got, want), (back, _diff(got, want)[:8])
        assert _same(_sweep(ctx, A, ref["x"], ref["b_fixed"], back, p), ref["x"]), ("fixed point", back)
    assert not _same(ref["fwd"], ref["bwd"]) or ref["colour"].max() == 0


Q = 16  # the integer twin's off-diagonals are -1 / Q


def _int_twin(A):
    """A's pattern with off-diagonals -1 / Q and a unit diagonal: 1 / a_ii = 1 and every product
    is a power-of-two scaling, so a sweep of integer data stays in the multiples of Q^-C after C
    colours -- exact in fp64 while they fit 53 bits (_exact_sweep checks that they do)."""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    assert np.all(np.bincount(rows[A.indices == rows], minlength=A.shape[0]) == 1)  # stored diagonals
    return sp.csr_matrix((np.where(A.indices == rows, 1.0, -1.0 / Q), A.indices.copy(), A.indptr.copy()),
                         shape=A.shape)


def _exact_sweep(T, colour, x, b, backward):
    """The sweep of the integer twin in int64, everything scaled by Q^C: row i of the colour gets
    X_i = B_i + (sum of its neighbours' X) / Q (x_i + (b_i - (x_i - sum / Q))).  The division is
    exact, and every partial sum of the kernel's row_dot stays below 2^53 in the scaled units."""
    nc = int(colour.max()) + 1
    scale = Q ** nc
    P = sp.csr_matrix(((T.data != 1.0).astype(np.int64), T.indices, T.indptr), shape=T.shape)  # off-diagonals
    X, Bs = E._int(x) * scale, E._int(b) * scale
    for c in (range(nc - 1, -1, -1) if backward else range(nc)):
        rows = np.flatnonzero(colour == c)
        assert (P[rows] @ np.abs(X)).max(initial=0) // Q + np.abs(X).max() + np.abs(Bs).max() < 1 << 53
        s = P[rows] @ X
        assert np.all(s % Q == 0)
        X[rows] = Bs[rows] + s // Q
    assert np.abs(X).max() < 1 << 53
    return X.astype(np.float64) / float(scale)


@pytest.mark.parametrize("path", ["per-colour", "one-workgroup"])
@pytest.mark.parametrize("name", ["7pt", "upwind_lower", "rows_65", "path"])
def test_sweep_exact_integers(ctx, oracle, name, path):
    """Integers in [-8, 8] on the integer twin (27-pt's 15 colours would need Q^15 > 2^53)."""
    import raptor_amd as ra

    Asp = _ops(oracle)[name]
    T = _int_twin(Asp)
    colour = _ref(oracle, name)["colour"]  # the pattern's colouring
    n = T.shape[0]
    rng = np.random.Generator(np.random.PCG64(7))
    ix, ib = (rng.integers(-8, 9, size=n).astype(np.float64) for _ in range(2))
    A = _dev(ra, ctx, T)
    A.colour(M.SEED)
    assert np.array_equal(A.colours(), colour)
    for back in (False, True):
        want = _exact_sweep(T, colour, ix, ib, back)
        got = _sweep(ctx, A, ix, ib, back, PATHS[path])
        assert _same(got, want), (back, _diff(got, want)[:8])
        fixed = T @ ix  # exact: multiples of 1 / Q
        assert _same(_sweep(ctx, A, ix, fixed, back, PATHS[path]), ix)


@pytest.mark.parametrize("path", ["per-colour", "one-workgroup"])
@pytest.mark.parametrize("name", ["27pt", "hub", f"rows_{M.SLICE + 1}", "wave_colours"])
def test_sweep_poisoned_columns(ctx, oracle, name, path):
    """x[c] = inf, then nan: what the restated sweep leaves finite has the restated bits (a
    padded cell that were multiplied, or read, would put a NaN into a row the column cannot reach);
    what it leaves non-finite is non-finite."""
    import raptor_amd as ra

    ref = _ref(oracle, name)
    A = _dev(ra, ctx, ref["A"])
    A.colour(M.SEED)
    n = ref["A"].shape[0]
    seen_finite = seen_bad = 0
    for c in sorted({0, n // 2, n - 1} | set(E.poison_columns(ref["A"])[:2])):
        for bad in (np.inf, np.nan):
            xp = np.array(ref["x"])
            xp[c] = bad
            for back in (False, True):
                with np.errstate(invalid="ignore"):
                    want = M.sweep(ref["Ao"], ref["colour"], xp, ref["b"], back)
                got = _sweep(ctx, A, xp, ref["b"], back, PATHS[path])
                fin = np.isfinite(want)
                assert np.array_equal(bits(got)[fin], bits(want)[fin]), (c, bad, back)
                assert not np.any(np.isfinite(got[~fin])), (c, bad, back)
                seen_finite += int(fin.sum())
                seen_bad += int((~fin).sum())
    assert seen_finite > 0 and seen_bad > 0


def test_paths_agree_on_a_level_sized_operator(ctx, oracle):
    """7-pt 20^3 (8,000 rows, eight waves' worth of slices per colour and more): path 1 and path 2
    give identical bits, and the automatic path is one of them."""
    import raptor_amd as ra

    O = oracle
    Ao = O.gen_7pt(20, 20, 20)
    n = Ao.shape[0]
    assert n <= M.WG_ROWS <= M.WG_CAPACITY
    A = ra.par_stencil_grid(ctx, "7pt", (20, 20, 20))
    colour, _ = M.first_fit(Ao.to_scipy(), M.SEED)
    A.colour(M.SEED)
    assert np.array_equal(A.colours(), colour)
    x, b = O.vec_uniform(n, 3), O.vec_uniform(n, 4)
    for back in (False, True):
        want = M.sweep(Ao, colour, x, b, back)
        res = [_sweep(ctx, A, x, b, back, p) for p in (1, 2, 0)]
        assert _same(res[0], res[1]) and _same(res[0], res[2]) and _same(res[0], want)


# ---- 3. the cycle ------------------------------------------------------------------------------------
# (problem, family): 7-pt 30 x 30 x 20 has level 0 over the one-workgroup threshold, the rest under it
CYCLE_CASES = [("7pt-big", "sa"), ("7pt-big", "pmis"), ("27pt", "sa"), ("7pt", "pmis")]
BIG = (30, 30, 20)
_CYC = {}


def _problem(O, what):
    if what == "7pt-big":
        Ao = O.gen_7pt(*BIG)
        return Ao, Ao.spmv(O.vec_uniform(Ao.shape[0], 42)), BIG
    Ao, b = K.problem(O, what)
    return Ao, b, K.PROBLEMS[what]


def _cycle_ref(O, what, fam, pre=1, post=1):
    key = (what, fam, pre, post)
    if key not in _CYC:
        Ao, b, dims = _problem(O, what)
        Ho = M.hierarchy(O, Ao, fam)
        S = M.mc_scaffold(O, Ho, pre, post)
        n = b.size
        xs, x = [], np.zeros(n)
        for _ in range(5):
            x = S.cycle(x, b)
            xs.append(_frozen(x))
        _CYC[key] = dict(Ao=Ao, b=_frozen(b), dims=dims, Ho=Ho, S=S, cycles=xs,
                         kind="7pt" if what.startswith("7pt") else "27pt")
    return _CYC[key]


def _hist_close(h, ho, rel):
    return h.shape == ho.shape and bool(np.all(np.abs(h - ho) <= rel * ho))


def _within_ulps(h, want, ulps):
    return h.shape == want.shape and bool(np.all(np.abs(h - want) <= ulps * np.spacing(want)))


@pytest.mark.parametrize("what,fam", CYCLE_CASES)
def test_levels_fall_on_both_sides_of_the_threshold(ctx, oracle, what, fam):
    import raptor_amd as ra

    ref = _cycle_ref(oracle, what, fam)
    S, Ho = ref["S"], ref["Ho"]
    A = ra.par_stencil_grid(ctx, ref["kind"], ref["dims"])
    ml = ra.ParMultilevel(**M.product_options(fam)).setup(A)
    assert ml.num_levels == Ho.num_levels >= 3
    sides = set()
    for l in range(ml.num_levels - 1):
        Al = ml.level_matrix(l, "A")
        assert same_csr(Al.to_scipy_local(), Ho.matrix(l, "A")), l
        lc = ml.level_colours(l)
        assert lc["n_colours"] == S.colour[l].max() + 1, l
        assert np.array_equal(Al.colours(), S.colour[l]), l
        assert Al.colour_rounds() == S.rounds[l]
        assert lc["one_workgroup"] == (1 if Al.local_rows <= M.WG_ROWS else 0), l
        sides.add(lc["one_workgroup"])
    assert sides == ({0, 1} if what == "7pt-big" else {1})
    for l in (ml.num_levels - 1, ml.num_levels, -1):
        with pytest.raises(ra.AmgError):
            ml.level_colours(l)
    with pytest.raises(ra.AmgError):  # another smoother has no colourings
        ra.ParMultilevel(**K.product_options("jacobi")).setup(A).level_colours(0)


@pytest.mark.parametrize("pre,post", [(1, 1), (2, 1), (0, 2)])
@pytest.mark.parametrize("what,fam", CYCLE_CASES[:2])
def test_sweep_counts(ctx, oracle, what, fam, pre, post):
    import raptor_amd as ra

    ref = _cycle_ref(oracle, what, fam, pre, post)
    A = ra.par_stencil_grid(ctx, ref["kind"], ref["dims"])
    ml = ra.ParMultilevel(**M.product_options(fam, pre, post)).setup(A)
    dx, db = ctx.zeros(ref["b"].size), _up(ctx, ref["b"])
    for k in range(3):
        ml.cycle(dx, db)
        assert _same(to_host(ctx, dx), ref["cycles"][k]), (k, pre, post)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("what,fam", CYCLE_CASES)
def test_cycles_solve_and_pcg_bit_exact(ctx, oracle, what, fam, graph):
    """Five cycles, a solve that stops on its tolerance, ten PCG iterations and five more cycles
    on one solver: the graphs are captured once and reused across the calls."""
    import raptor_amd as ra

    O = oracle
    ref = _cycle_ref(O, what, fam)
    S, Ao, b = ref["S"], ref["Ao"], ref["b"]
    n = b.size
    A = ra.par_stencil_grid(ctx, ref["kind"], ref["dims"])
    ml = ra.ParMultilevel(use_graph=graph, **M.product_options(fam)).setup(A)
    assert ml.graph_enabled == graph
    db = _up(ctx, b)

    def five():
        dx = ctx.zeros(n)
        for k in range(5):
            ml.cycle(dx, db)
            got = to_host(ctx, dx)
            assert _same(got, ref["cycles"][k]), ("cycle", k, _diff(got, ref["cycles"][k])[:8])

    five()
    # solve: stops where the scaffold stops, with its iterate
    tol = 1e-6
    xo, ho = S.solve(np.zeros(n), b, max_iter=40, tol=tol)
    assert 2 <= len(ho) - 1 < 40 and np.all(np.abs(ho / ho[0] - tol) >= 0.01 * tol)
    dx = ctx.zeros(n)
    _, h = ml.solve(dx, db, max_iter=40, tol=tol)
    assert len(h) == len(ho) and _same(to_host(ctx, dx), xo)
    assert _hist_close(h, ho, 1e-10), (h, ho)
    # PCG on the (symmetric) cycle, the product's dot tree
    xr, rr = K.pcg_restated(S, Ao, np.zeros(n), b, 10, 0.0, K.dot_tree)
    dx = ctx.zeros(n)
    _, h = ml.pcg(dx, db, max_iter=10)
    assert _same(to_host(ctx, dx), xr)
    assert _within_ulps(h, np.sqrt(rr), SQRT_ULPS), (h, np.sqrt(rr))
    assert h[-1] < 1e-4 * h[0]
    five()


_BICG = {}


def _bicg_ref(O, cuts=None):
    """Convection-diffusion (cell Peclet 8): six BiCGStab iterations on the restated cycle."""
    key = tuple(cuts) if cuts else None
    if "base" not in _BICG:
        csr = B.convdiff(*B.GRIDS[1], 8.0)
        Ao = B.oracle_matrix(O, csr)
        b = _frozen(B.rhs(O, Ao.shape[0]))
        Ho = M.hierarchy(O, Ao, "pmis", max_coarse=B.MAX_COARSE)
        _BICG["base"] = (csr, Ao, b, Ho, M.mc_scaffold(O, Ho))
    csr, Ao, b, Ho, S = _BICG["base"]
    if key not in _BICG:
        dot = (lambda u, v: K.dot_tree(u, v, cuts)) if cuts else K.dot_tree
        x, rr, st = B.bicgstab_restated(S, Ao, np.zeros(b.size), b, 6, 0.0, dot)
        _BICG[key] = (_frozen(x), np.sqrt(rr), st)
    return (csr, Ao, b, Ho, S) + _BICG[key]


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_bicgstab_bit_exact(ctx, oracle, graph):
    import raptor_amd as ra

    csr, Ao, b, Ho, S, xr, hr, st = _bicg_ref(oracle)
    A = _dev(ra, ctx, sp.csr_matrix((csr[2], csr[1], csr[0]), shape=Ao.shape))
    ml = ra.ParMultilevel(use_graph=graph, **M.product_options("pmis", max_coarse=B.MAX_COARSE)).setup(A)
    assert ml.num_levels == Ho.num_levels >= 3
    db = _up(ctx, b)
    for _ in range(2):  # the second call replays the first call's graphs
        dx = ctx.zeros(b.size)
        _, h, status = ml.bicgstab(dx, db, max_iter=6)
        assert status == st == B.KRYLOV_OK and _same(to_host(ctx, dx), xr)
        assert _within_ulps(h, hr, SQRT_ULPS), (h, hr)
    assert hr[-1] < 1e-3 * hr[0]


# ---- 4. partition independence -----------------------------------------------------------------
@pytest.mark.parametrize("rep", [0, 10 ** 9], ids=["distributed", "rep-all"])
@pytest.mark.parametrize("what,fam", [("7pt", "pmis"), ("27pt", "sa")])
@pytest.mark.parametrize("nranks", [2, 3])
def test_cycle_solve_pcg_on_loopback_ranks(oracle, nranks, what, fam, rep):
    """Every rank's slice of five cycles, of a solve that stops on its tolerance and of ten PCG
    iterations is the one-rank restatement's (the dot tree cut at the ranks' rows)."""
    import raptor_amd as ra

    O = oracle
    ref = _cycle_ref(O, what, fam)
    S, Ao, b = ref["S"], ref["Ao"], ref["b"]
    n = b.size
    tol = 1e-6
    xo, ho = S.solve(np.zeros(n), b, max_iter=40, tol=tol)

    def rank(r, nr, world):
        c = loopback_ctx(r, nr, world)
        A = ra.par_stencil_grid(c, ref["kind"], ref["dims"])
        ml = ra.ParMultilevel(replicate_below=rep, **M.product_options(fam)).setup(A)
        lo, cnt = A.first_row, A.local_rows
        db = _up(c, b[lo:lo + cnt])
        dx, xs = c.zeros(cnt), []
        for _ in range(5):
            ml.cycle(dx, db)
            xs.append(to_host(c, dx))
        dx = c.zeros(cnt)
        _, h = ml.solve(dx, db, max_iter=40, tol=tol)
        sx = to_host(c, dx)
        dx = c.zeros(cnt)
        _, hp = ml.pcg(dx, db, max_iter=10)
        cols = [ml.level_colours(l) for l in range(ml.num_levels - 1)]
        return ml.num_levels, lo, cnt, xs, h, sx, hp, to_host(c, dx), cols

    res = run_ranks(nranks, rank)
    starts = [lo for _, lo, *_ in res] + [n]
    assert starts == sorted(starts) and sum(r[2] for r in res) == n
    xr, rr = K.pcg_restated(S, Ao, np.zeros(n), b, 10, 0.0, lambda u, v: K.dot_tree(u, v, starts))
    for nl, lo, cnt, xs, h, sx, hp, px, cols in res:
        assert nl == ref["Ho"].num_levels
        for k in range(5):
            assert _same(xs[k], ref["cycles"][k][lo:lo + cnt]), ("cycle", k, lo)
        assert len(h) == len(ho) and _same(sx, xo[lo:lo + cnt]) and _hist_close(h, ho, 1e-10)
        assert _same(px, xr[lo:lo + cnt]) and _within_ulps(hp, np.sqrt(rr), SQRT_ULPS)
        assert [c["n_colours"] for c in cols] == [int(c.max()) + 1 for c in S.colour]
        # a distributed level sweeps colour by colour (its launches follow halo exchanges)
        assert cols[0]["one_workgroup"] == 0
        assert all(c["one_workgroup"] == (1 if rep else 0) for c in cols[1:])


@pytest.mark.parametrize("nranks", [2, 3])
def test_bicgstab_on_loopback_ranks(oracle, nranks):
    import raptor_amd as ra

    O = oracle
    csr = _bicg_ref(O)[0]
    n = csr[0].size - 1
    cuts = B.ragged_cuts(n, nranks)
    _, Ao, b, Ho, S, xr, hr, st = _bicg_ref(O, cuts)
    Asp = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(n, n))

    def rank(r, nr, world):
        c = loopback_ctx(r, nr, world)
        lo, hi = cuts[r], cuts[r + 1]
        A = _dev(ra, c, Asp, lo, hi)
        ml = ra.ParMultilevel(replicate_below=0, **M.product_options("pmis", max_coarse=B.MAX_COARSE)).setup(A)
        dx = c.zeros(hi - lo)
        _, h, status = ml.bicgstab(dx, _up(c, b[lo:hi]), max_iter=6)
        return to_host(c, dx), h, status

    for r, (x, h, status) in enumerate(run_ranks(nranks, rank)):
        assert status == st and _same(x, xr[cuts[r]:cuts[r + 1]]), r
        assert _within_ulps(h, hr, SQRT_ULPS)


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("name", ["hub", "upwind_lower", "wave_colours"])
def test_sweep_on_loopback_ranks(oracle, name, nranks):
    """The per-colour sweep with its halo exchanges: every rank's slice of a forward and a
    backward sweep is the one-rank restatement's; the one-workgroup path refuses."""
    import raptor_amd as ra

    ref = _ref(oracle, name)
    Asp = ref["A"]
    cuts = M.cuts(Asp.shape[0], nranks)

    def rank(r, nr, world):
        c = loopback_ctx(r, nr, world)
        lo, hi = cuts[r], cuts[r + 1]
        A = _dev(ra, c, Asp, lo, hi)
        A.colour(M.SEED)
        out = [_sweep(c, A, ref["x"][lo:hi], ref["b"][lo:hi], back, 0) for back in (False, True)]
        with pytest.raises(ra.AmgError):
            A.mc_gs(_up(c, ref["x"][lo:hi]), _up(c, ref["b"][lo:hi]), path=2)
        return out

    for r, (f, bw) in enumerate(run_ranks(nranks, rank)):
        lo, hi = cuts[r], cuts[r + 1]
        assert _same(f, ref["fwd"][lo:hi]) and _same(bw, ref["bwd"][lo:hi]), r


# ---- 5. error paths ------------------------------------------------------------------------------
def test_error_paths_leave_the_context_usable(ctx, oracle):
    import raptor_amd as ra

    ref = _ref(oracle, "27pt")
    n = ref["A"].shape[0]
    A = _dev(ra, ctx, ref["A"])
    dx, db = _up(ctx, ref["x"]), _up(ctx, ref["b"])
    with pytest.raises(ra.AmgError):   # a sweep before colour
        A.mc_gs(dx, db)
    with pytest.raises(ra.AmgError):
        A.colours()
    assert _same(to_host(ctx, dx), ref["x"])
    A.colour(M.SEED)
    with pytest.raises(ra.AmgError):   # x overlapping b: the same vector, and a shifted view
        A.mc_gs(dx, dx)
    buf = _up(ctx, np.concatenate([ref["x"], ref["b"]]))
    with pytest.raises(ra.AmgError):
        A.mc_gs(buf[:n], buf[n - 1:2 * n - 1])
    with pytest.raises(ra.AmgError):   # no such path
        A.mc_gs(dx, db, path=3)
    assert _same(to_host(ctx, dx), ref["x"])
    A.mc_gs(buf[:n], buf[n:])          # adjacent, not overlapping
    assert _same(to_host(ctx, buf)[:n], ref["fwd"]) and _same(to_host(ctx, buf)[n:], ref["b"])
    # beyond the one-workgroup capacity: path 2 refuses, the other paths sweep
    big = ra.par_stencil_grid(ctx, "7pt", BIG)
    nb = big.local_rows
    assert nb > M.WG_CAPACITY
    big.colour(M.SEED)
    O = oracle
    Ao = O.gen_7pt(*BIG)
    x, b = O.vec_uniform(nb, 3), O.vec_uniform(nb, 4)
    dx = _up(ctx, x)
    with pytest.raises(ra.AmgError):
        big.mc_gs(dx, _up(ctx, b), path=2)
    assert _same(to_host(ctx, dx), x)
    colour, _ = M.first_fit(Ao.to_scipy(), M.SEED)
    for p in (0, 1):
        assert _same(_sweep(ctx, big, x, b, False, p), M.sweep(Ao, colour, x, b))
    with pytest.raises(ra.AmgError):   # colourings are of square operators
        ml = ra.ParMultilevel(**K.product_options("jacobi")).setup(ra.par_stencil_grid(ctx, "7pt", (8, 8, 8)))
        ml.level_matrix(0, "P").colour(M.SEED)
