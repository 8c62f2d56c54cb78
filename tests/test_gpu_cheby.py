"""The Chebyshev smoother on the GPU (KM_CHEBY in kernels.hip, Solver::setup_cheby in
solver_setup.hip, Solver::smooth in multilevel.hip) against the restatement of
tests/cheby_cases.py (checked on the CPU by tests/test_cheby_cpu.py), exact int64 arithmetic, exact fixed points and poisoned columns.

Bars: chebyshev_step, level_eig, V-cycle, solve and PCG iterates bit-identical (edge_cases.bits);
solve histories within 1e-10 relative, entries left by a fused norm within 1e-12; PCG history
entries within SQRT_ULPS of sqrt(rr_k) (tests/test_gpu_cycle_options.py).  Small shapes only."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import cheby_cases as CH
from tests import cycle_option_cases as K
from tests import edge_cases as E
from tests.edge_cases import bits
from tests.test_gpu_cycle_options import SQRT_ULPS
from tests.test_gpu_kernel_edges import CONFIGS, DIAG_NAMES, STENCILS, TPL_PATHS
from tests.test_gpu_multirank import run_ranks
from tests.util import loopback_ctx, same_csr, to_dev, to_host

pytestmark = pytest.mark.gpu

C1, C2 = 0.37109375, 0.8125  # any coefficients: the level kernel takes them as arguments


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


def _diff(a, b):
    return np.flatnonzero(bits(a) != bits(b))


def _frozen(a):
    a = np.array(a, np.float64)
    a.setflags(write=False)
    return a


def _up(ctx, a):
    return to_dev(ctx, np.array(a, np.float64))


def _dev(ra, ctx, A):
    return ra.ParCSRMatrix.from_csr(ctx, A.shape[0], 0, A.indptr, A.indices, A.data)


def _orc(O, A):
    return O.Csr.from_arrays(A.shape[0], A.shape[1], A.indptr, A.indices, A.data)


def _setenv(monkeypatch, *envs):
    for env in envs:
        for k, v in env.items():
            monkeypatch.setenv(k, v)


def exact_cheby(A, x, xprev, b):
    """c1 = c2 = 0.5, power-of-two a_ii = d: x' = (2 d x + d (x - xprev) + r) / (2 d), r = b - A x,
    the numerator in int64 (every intermediate of the kernel's expression is then exact too:
    (x - xprev) / 2, r / (2 d) and their sum are integers over 2 d below 2^53)."""
    E.assert_exact_range(A, x, b)
    d = E._int(A.diagonal())
    assert np.all(d > 0) and np.all(d & (d - 1) == 0), "diagonal must be a positive power of two"
    xi, pi = E._int(x), E._int(xprev)
    r = E._int(b) - E._imat(A) @ xi
    num = xi * (2 * d) + d * (xi - pi) + r
    assert np.abs(num).max(initial=0) < 1 << 53 and np.abs(d * (xi - pi) + r).max(initial=0) < 1 << 53
    return num.astype(np.float64) / (2 * d).astype(np.float64)


def _three_calls(ctx, A, x, xprev, b, c1, c2):
    """chebyshev_step with x_prev given, x_prev None and x_out aliased to x_prev."""
    n = x.size
    dx, db, dp = _up(ctx, x), _up(ctx, b), _up(ctx, xprev)
    given = to_host(ctx, A.chebyshev_step(dx, dp, db, ctx.empty(n), c1, c2))
    assert _same(to_host(ctx, dp), xprev) and _same(to_host(ctx, dx), x)  # operands untouched
    none = to_host(ctx, A.chebyshev_step(dx, None, db, ctx.empty(n), c1, c2))
    alias = to_host(ctx, A.chebyshev_step(dx, dp, db, dp, c1, c2))
    return given, none, alias


_REFS = {}


def _step_refs(O, key, Asp, exact):
    """Per operator, once: the restated step on vec_uniform data (x_prev given and zeros) and,
    for integer operators, the int64 result and the fixed-point right-hand side."""
    if key in _REFS:
        return _REFS[key]
    Ao = _orc(O, Asp)
    n = Asp.shape[0]
    dinv = 1.0 / Asp.diagonal()
    x, b, xp = O.vec_uniform(n, 3), O.vec_uniform(n, 4), O.vec_uniform(n, 5)
    ref = dict(Ao=Ao, dinv=dinv, x=x, b=b, xp=xp,
               given=CH.cheby_step(Ao, dinv, x, xp, b, C1, C2),
               none=CH.cheby_step(Ao, dinv, x, np.zeros(n), b, C1, C2))
    if exact:
        ix, iy0, ib = E.int_vectors(n, 7)
        ref.update(ix=ix, ip=iy0, ib=ib, exact=exact_cheby(Asp, ix, iy0, ib),
                   exact_none=exact_cheby(Asp, ix, np.zeros(n), ib), b_fixed=E.b_for_fixed_point(Asp, ix))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _REFS[key] = ref
    return ref


def _check_step(ctx, A, ref, exact):
    given, none, alias = _three_calls(ctx, A, ref["x"], ref["xp"], ref["b"], C1, C2)
    assert _same(given, ref["given"]), ("x_prev", _diff(given, ref["given"])[:8])
    assert _same(none, ref["none"]), ("NULL", _diff(none, ref["none"])[:8])
    assert _same(alias, ref["given"]), ("aliased", _diff(alias, ref["given"])[:8])
    assert not _same(ref["given"], ref["none"])
    if not exact:
        return
    given, none, alias = _three_calls(ctx, A, ref["ix"], ref["ip"], ref["ib"], 0.5, 0.5)
    assert _same(given, ref["exact"]), ("exact", _diff(given, ref["exact"])[:8])
    assert _same(none, ref["exact_none"]) and _same(alias, ref["exact"])
    # fixed points: b = A x in int64 and x_prev = x return x, whatever the coefficients
    x = ref["ix"]
    for c1, c2 in ((C1, C2), (-0.25, 1.75)):
        given, _, alias = _three_calls(ctx, A, x, x, ref["b_fixed"], c1, c2)
        assert _same(given, x) and _same(alias, x), (c1, c2)


def _check_poison(ctx, A, Asp, ref, cols):
    """x[c] = inf, then nan: every row without an entry in column c has the restated bits."""
    n = Asp.shape[0]
    db, dp = _up(ctx, ref["b"]), _up(ctx, ref["xp"])
    for c in cols:
        keep = E.rows_without(Asp, c)
        for bad in (np.inf, np.nan):
            xp = np.array(ref["x"])
            xp[c] = bad
            got = to_host(ctx, A.chebyshev_step(_up(ctx, xp), dp, db, ctx.empty(n), C1, C2))
            with np.errstate(invalid="ignore"):
                want = CH.cheby_step(ref["Ao"], ref["dinv"], xp, ref["xp"], ref["b"], C1, C2)
            wrong = np.flatnonzero(bits(got)[keep] != bits(want)[keep])
            assert wrong.size == 0, (c, bad, np.flatnonzero(keep)[wrong][:8])


# ---- 1. chebyshev_step on the format zoo -------------------------------------------------------
@pytest.mark.parametrize("fmt,var", CONFIGS, ids=[f if v is None else f"{f}-v{v}" for f, v in CONFIGS])
@pytest.mark.parametrize("name", DIAG_NAMES)
def test_zoo_chebyshev_step(ctx, oracle, monkeypatch, name, fmt, var):
    import raptor_amd as ra

    c = E.zoo()[name]
    _setenv(monkeypatch, c.env, {} if var is None else {"AMG_KERNEL_VARIANT": var})
    A = _dev(ra, ctx, c.A).set_format(fmt)
    assert A.info["n_blocks"] == c.n_blocks
    if c.n_templates is not None:
        assert A.info["template_rows"] == (c.template_rows if fmt == "auto" else 0)
    ref = _step_refs(oracle, name, c.A, True)
    _check_step(ctx, A, ref, True)
    _check_poison(ctx, A, c.A, ref, E.poison_columns(c.A))


@pytest.mark.parametrize("name", ["cap_nnz_plus1", "vi_255_256_257", "gs_chain_63"])
def test_step_notices_one_changed_entry(ctx, oracle, monkeypatch, name):
    """1 added to one stored off-diagonal value, or to one x_prev entry: exactly that row differs
    from the int64 result, and the fixed point is lost there."""
    import raptor_amd as ra

    c = E.zoo()[name]
    ref = _step_refs(oracle, name, c.A, True)
    _setenv(monkeypatch, c.env)
    Am = c.A.copy()
    n = c.A.shape[0]
    r = n // 2
    k = Am.indptr[r] + (1 if Am.indices[Am.indptr[r]] == r else 0)
    assert Am.indices[k] != r
    Am.data[k] += 1.0
    A = _dev(ra, ctx, Am)
    given, none, alias = _three_calls(ctx, A, ref["ix"], ref["ip"], ref["ib"], 0.5, 0.5)
    assert _diff(given, ref["exact"]).tolist() == _diff(alias, ref["exact"]).tolist() == [r]
    assert _diff(none, ref["exact_none"]).tolist() == [r]
    x = ref["ix"]
    given, _, _ = _three_calls(ctx, A, x, x, ref["b_fixed"], C1, C2)
    assert _diff(given, x).tolist() == [r]
    # the unchanged operator, one changed x_prev entry
    A = _dev(ra, ctx, c.A)
    for q in (0, r, n - 1):
        xp = np.array(ref["ip"])
        xp[q] += 2.0
        given, _, alias = _three_calls(ctx, A, ref["ix"], xp, ref["ib"], 0.5, 0.5)
        assert _diff(given, ref["exact"]).tolist() == _diff(alias, ref["exact"]).tolist() == [q]


# ---- 2. the template kernels -------------------------------------------------------------------
def _int_stencil(kind, dims):
    """The 7- or 27-point stencil with off-diagonals -1 and a power-of-two diagonal (8 / 32):
    integer entries for the exact checks, the same row shapes as the oracle's generators."""
    nx, ny, nz = dims

    def band(m, corner):
        return sp.diags([np.ones(m - 1), np.ones(m), np.ones(m - 1)], [-1, 0, 1]) if corner else \
            sp.diags([np.ones(m - 1), np.ones(m - 1)], [-1, 1])

    if kind == "27pt":
        A = -sp.kron(band(nz, True), sp.kron(band(ny, True), band(nx, True)))
        A = A + sp.identity(nx * ny * nz) * 33.0
    else:
        ex, ey, ez = sp.identity(nx), sp.identity(ny), sp.identity(nz)
        A = -(sp.kron(ez, sp.kron(ey, band(nx, False))) + sp.kron(ez, sp.kron(band(ny, False), ex)) +
              sp.kron(band(nz, False), sp.kron(ey, ex))) + sp.identity(nx * ny * nz) * 8.0
    A = A.tocsr()
    A.sort_indices()
    A.eliminate_zeros()
    return A


@pytest.mark.parametrize("path", list(TPL_PATHS))
@pytest.mark.parametrize("kind,dims", STENCILS, ids=[f"{k}-{'x'.join(map(str, d))}" for k, d in STENCILS])
def test_stencil_chebyshev_step(ctx, oracle, monkeypatch, kind, dims, path):
    """The row-template kernels -- uniform stencil, per-template tables, the forced march -- on
    the oracle's stencil (restatement, poisoned columns) and on its integer twin (int64, fixed
    points)."""
    import raptor_amd as ra

    O = oracle
    _setenv(monkeypatch, TPL_PATHS[path])
    Asp = {"7pt": O.gen_7pt, "27pt": O.gen_27pt}[kind](*dims).to_scipy()
    Ai = _int_stencil(kind, dims)
    assert np.array_equal(Ai.indptr, Asp.indptr) and np.array_equal(Ai.indices, Asp.indices)
    assert set(Ai.diagonal()) == {8.0 if kind == "7pt" else 32.0}
    n = Asp.shape[0]
    groups = [(q, min(n, q + 512)) for q in range(0, n, 512)]
    for M, exact in ((Asp, False), (Ai, True)):
        A = _dev(ra, ctx, M)
        inf = A.info
        assert inf["template_rows"] == n > 0
        assert inf["tpl_master"] == (0 if path == "generic" else {"7pt": 7, "27pt": 27}[kind])
        if path == "march" and dims == (260, 8, 8):
            assert inf["tpl_march_shift"] > 0
        ref = _step_refs(O, (kind, dims, exact), M, exact)
        _check_step(ctx, A, ref, exact)
        _check_poison(ctx, A, M, ref, E.poison_columns(M, groups))


# ---- 3. lambda_l -------------------------------------------------------------------------------
_HIER = {}


def _hier(O, kind, fam):
    if (kind, fam) not in _HIER:
        Ao, b, Ho = CH.hierarchy(O, kind, fam)
        lam = []
        for l in range(Ho.num_levels - 1):
            A = Ho.matrix(l, "A")
            lam.append(O.sa_rho(O.Csr.from_scipy(A), A.diagonal(), CH.SEED + l))
        _HIER[kind, fam] = (Ao, _frozen(b), Ho, lam)
    return _HIER[kind, fam]


@pytest.mark.parametrize("kind", list(K.PROBLEMS))
@pytest.mark.parametrize("fam", CH.FAMILIES)
def test_level_eig_one_rank(ctx, oracle, kind, fam):
    import raptor_amd as ra

    _, _, Ho, lam = _hier(oracle, kind, fam)
    A = ra.par_stencil_grid(ctx, kind, K.PROBLEMS[kind])
    ml = ra.ParMultilevel(**CH.product_options(fam)).setup(A)
    assert ml.num_levels == Ho.num_levels >= 4
    got = [ml.level_eig(l) for l in range(ml.num_levels - 1)]
    assert _same(got, lam), (got, lam)


@pytest.mark.parametrize("rep", [0, 800, 10 ** 9], ids=["distributed", "rep-800", "rep-all"])
@pytest.mark.parametrize("fam", CH.FAMILIES)
@pytest.mark.parametrize("nranks", [2, 3])
def test_level_eig_loopback_ranks(oracle, nranks, fam, rep):
    """Ragged row cuts; levels distributed, replicated from the first level of <= 800 rows on,
    or all replicated below level 0: every rank reports the one-rank lambda_l."""
    import raptor_amd as ra

    Ao, _, Ho, lam = _hier(oracle, "7pt", fam)
    M = Ao.to_scipy()
    n = M.shape[0]
    cuts = {2: [0, 1237, n], 3: [0, 37, 1901, n]}[nranks]

    def rank(r, nr, world):
        c = loopback_ctx(r, nr, world)
        lo, hi = cuts[r], cuts[r + 1]
        A = ra.ParCSRMatrix.from_scipy_local(c, M[lo:hi], n, lo)
        ml = ra.ParMultilevel(replicate_below=rep, **CH.product_options(fam)).setup(A)
        sizes = [ml.level_info(l)["n_local"] for l in range(ml.num_levels)]
        return ml.num_levels, [ml.level_eig(l) for l in range(ml.num_levels - 1)], sizes

    res = run_ranks(nranks, rank)
    glob = [Ho.matrix(l, "A").shape[0] for l in range(Ho.num_levels)]
    for nl, got, sizes in res:
        assert nl == Ho.num_levels
        assert _same(got, lam), (got, lam)
        if rep:  # the replicated levels are whole on the rank
            whole = [l for l in range(1, nl) if glob[l] <= rep]
            assert whole and all(sizes[l] == glob[l] for l in whole)


# ---- 4. cycle options --------------------------------------------------------------------------
_CYCLE_REFS = {}


def _cycle_ref(O, kind, fam, pre, post, m, f):
    key = (kind, fam, pre, post, m, f)
    if key not in _CYCLE_REFS:
        _, b, Ho, lam = _hier(O, kind, fam)
        S = CH.cheby_scaffold(O, Ho, pre, post, m, f)
        assert _same(S.lam, lam)
        n = b.size
        xs, x = [], np.zeros(n)
        for _ in range(4):
            x = S.cycle(x, b)
            xs.append(_frozen(x))
        sx, sh = S.solve(np.zeros(n), b, max_iter=6)
        mats = [(Ho.matrix(l, "A"), Ho.matrix(l, "P"), Ho.matrix(l, "R")) for l in range(Ho.num_levels)]
        _CYCLE_REFS[key] = dict(b=b, mats=mats, cycles=xs, solve_x=_frozen(sx), solve_hist=_frozen(sh))
    return _CYCLE_REFS[key]


def _hist_close(h, ho, rel):
    return h.shape == ho.shape and bool(np.all(np.abs(h - ho) <= rel * ho))


@pytest.mark.parametrize("case", CH.gpu_matrix(), ids=CH.case_id)
def test_cheby_cycle_options_bit_exact(ctx, oracle, monkeypatch, case):
    """Every (pre, post, degree, fraction): the hierarchy is the oracle's, four V-cycles from
    x = 0 and a 6-cycle solve are the restated cycle's bit for bit, replayed from graphs and
    launched eagerly; the byte model follows the sweep counts and the degree."""
    import raptor_amd as ra

    kind, env, fam, pre, post, m, f = case
    _setenv(monkeypatch, K.ENVS[env])
    ref = _cycle_ref(oracle, kind, fam, pre, post, m, f)
    A = ra.par_stencil_grid(ctx, kind, K.PROBLEMS[kind])
    n = A.local_rows
    db = to_dev(ctx, ref["b"])
    for graph in (True, False):
        ml = ra.ParMultilevel(use_graph=graph, **CH.product_options(fam, pre, post, m, f)).setup(A)
        assert ml.graph_enabled == graph
        if graph:
            assert ml.num_levels == len(ref["mats"]) >= 4
            for l, (Al, Pl, Rl) in enumerate(ref["mats"]):
                assert same_csr(ml.level_matrix(l, "A").to_scipy_local(), Al), ("A", l)
                if l + 1 < ml.num_levels:
                    assert same_csr(ml.level_matrix(l, "P").to_scipy_local(), Pl), ("P", l)
                    assert same_csr(ml.level_matrix(l, "R").to_scipy_local(), Rl), ("R", l)
            infos = [ml.level_info(l) for l in range(ml.num_levels)]
            for l in range(ml.num_levels):
                assert infos[l]["bytes_per_cycle_local"] == CH.bytes_model(infos, l, pre, post, m), ("bytes", l)
            if env == "tpl":
                assert A.info["template_rows"] > 0
        dx = ctx.zeros(n)
        for k in range(4):
            ml.cycle(dx, db)
            got = to_host(ctx, dx)
            assert _same(got, ref["cycles"][k]), ("cycle", k, graph, _diff(got, ref["cycles"][k])[:8])
        dx = ctx.zeros(n)
        _, hist = ml.solve(dx, db, max_iter=6)
        assert _same(to_host(ctx, dx), ref["solve_x"]), ("solve", graph)
        print(case, graph, "history error", np.max(np.abs(hist - ref["solve_hist"]) / ref["solve_hist"]))
        assert _hist_close(hist, ref["solve_hist"], 1e-10), (graph, hist, ref["solve_hist"])
        if pre >= 1:  # every entry but the last left by a cycle's first step (fused norm)
            assert _hist_close(hist, ref["solve_hist"], 1e-12), (graph, hist, ref["solve_hist"])


# ---- 5. partition independence -----------------------------------------------------------------
@pytest.mark.parametrize("rep", [0, 10 ** 9], ids=["distributed", "rep-all"])
@pytest.mark.parametrize("fam,pre,post,m,f", [("pmis", 1, 1, 2, 0.3), ("sa", 2, 1, 3, 0.1), ("sa", 0, 1, 4, 0.3)])
@pytest.mark.parametrize("nranks", [2, 3])
def test_cheby_cycle_is_partition_independent(oracle, nranks, fam, pre, post, m, f, rep):
    """Loopback ranks: every rank's slice of three V-cycles is the one-rank restatement's; no
    rank cut is passed to anything."""
    import raptor_amd as ra

    kind = "7pt"
    ref = _cycle_ref(oracle, kind, fam, pre, post, m, f)
    b = ref["b"]

    def rank(r, nr, world):
        c = loopback_ctx(r, nr, world)
        A = ra.par_stencil_grid(c, kind, K.PROBLEMS[kind])
        ml = ra.ParMultilevel(replicate_below=rep, **CH.product_options(fam, pre, post, m, f)).setup(A)
        lo, cnt = A.first_row, A.local_rows
        dx, db = c.zeros(cnt), to_dev(c, b[lo:lo + cnt])
        xs = []
        for _ in range(3):
            ml.cycle(dx, db)
            xs.append(to_host(c, dx))
        return ml.num_levels, lo, cnt, xs

    res = run_ranks(nranks, rank)
    assert sum(cnt for _, _, cnt, _ in res) == b.size
    for nl, lo, cnt, xs in res:
        assert nl == len(ref["mats"])
        for k in range(3):
            assert _same(xs[k], ref["cycles"][k][lo:lo + cnt]), ("cycle", k, lo)


# ---- 6. PCG and stopping -----------------------------------------------------------------------
def _within_ulps(h, want, ulps):
    return h.shape == want.shape and bool(np.all(np.abs(h - want) <= ulps * np.spacing(want)))


@pytest.mark.parametrize("m,f", [(2, 0.3), (3, 0.1)])
@pytest.mark.parametrize("kind", list(K.PROBLEMS))
@pytest.mark.parametrize("fam", CH.FAMILIES)
def test_cheby_pcg_bit_exact_on_the_dot_tree(ctx, oracle, fam, kind, m, f):
    """Ten PCG iterations preconditioned by the (symmetric) Chebyshev cycle give the x of the
    restated loop on the product's dot tree, graphs on and off; the history is sqrt(rr_k)."""
    import raptor_amd as ra

    O = oracle
    Ao, b, Ho, _ = _hier(O, kind, fam)
    S = CH.cheby_scaffold(O, Ho, 1, 1, m, f)
    n = b.size
    xr, rr = K.pcg_restated(S, Ao, np.zeros(n), b, 10, 0.0, K.dot_tree)
    want = np.sqrt(rr)
    assert want.shape == (11,) and np.all(want > 0) and want[-1] < 1e-3 * want[0]
    A = ra.par_stencil_grid(ctx, kind, K.PROBLEMS[kind])
    db = to_dev(ctx, b)
    for graph in (True, False):
        ml = ra.ParMultilevel(use_graph=graph, **CH.product_options(fam, 1, 1, m, f)).setup(A)
        dx = ctx.zeros(n)
        _, h = ml.pcg(dx, db, max_iter=10)
        assert _same(to_host(ctx, dx), xr), graph
        assert _within_ulps(h, want, SQRT_ULPS), (graph, h, want)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("fam,what", list(CH.STOP))
def test_cheby_tolerance_stops_at_the_restated_iteration(ctx, oracle, fam, what, graph):
    """solve / pcg with a tolerance stop where the restated loop stops (tests/test_cheby_cpu.py
    checks that no history ratio comes within 1 % of the tolerance), with its iterate."""
    import raptor_amd as ra

    O = oracle
    Ao, b, Ho, _ = _hier(O, "7pt", fam)
    S = CH.cheby_scaffold(O, Ho, 1, 1, 2, 0.3)
    n = b.size
    kw = CH.STOP[fam, what]
    A = ra.par_stencil_grid(ctx, "7pt", K.PROBLEMS["7pt"])
    ml = ra.ParMultilevel(use_graph=graph, **CH.product_options(fam)).setup(A)
    dx, db = ctx.zeros(n), to_dev(ctx, b)
    if what == "solve":
        xo, ho = S.solve(np.zeros(n), b, **kw)
        _, h = ml.solve(dx, db, **kw)
        assert len(h) == len(ho) and 1 < len(h) <= kw["max_iter"]
        assert _same(to_host(ctx, dx), xo)
        assert _hist_close(h, ho, 1e-10)
    else:
        xr, rr = K.pcg_restated(S, Ao, np.zeros(n), b, kw["max_iter"], kw["tol"], K.dot_tree)
        _, h = ml.pcg(dx, db, **kw)
        assert len(h) == len(rr) and 1 < len(h) <= kw["max_iter"]
        assert _same(to_host(ctx, dx), xr)
        assert _within_ulps(h, np.sqrt(rr), SQRT_ULPS), (h, np.sqrt(rr))
    assert h[-1] / h[0] < kw["tol"] and np.all(h[:-1] / h[0] >= kw["tol"])


# ---- 7. bad options and state ------------------------------------------------------------------
def test_bad_cheby_options_raise_and_leave_the_context_usable(ctx, oracle):
    import raptor_amd as ra

    O = oracle
    _, b, Ho, _ = _hier(O, "7pt", "pmis")
    A = ra.par_stencil_grid(ctx, "7pt", K.PROBLEMS["7pt"])
    bad = [dict(cheby_degree=0), dict(cheby_degree=17), dict(cheby_fraction=0.0),
           dict(cheby_fraction=1.0), dict(cheby_fraction=-0.1)]
    for kw in bad:
        with pytest.raises(ra.AmgError):
            ra.ParMultilevel(**dict(CH.product_options("pmis"), **kw)).setup(A)
    xo = O.Hierarchy(K.problem(O, "7pt")[0], **K.oracle_options(O, "jacobi")).cycle(np.zeros(b.size), b)
    for kw in bad:  # read only under Chebyshev: the other smoothers take any value
        ml = ra.ParMultilevel(**dict(K.product_options("jacobi"), **kw)).setup(A)
        dx = ctx.zeros(b.size)
        ml.cycle(dx, to_dev(ctx, b))
        assert _same(to_host(ctx, dx), xo), kw
        with pytest.raises(ra.AmgError):
            ml.level_eig(0)
    ml = ra.ParMultilevel(**CH.product_options("pmis")).setup(A)
    assert ml.level_eig(ml.num_levels - 2) > 0.0
    for l in (ml.num_levels - 1, ml.num_levels, -1):
        with pytest.raises(ra.AmgError):
            ml.level_eig(l)
    dx = ctx.zeros(b.size)
    ml.cycle(dx, to_dev(ctx, b))
    assert _same(to_host(ctx, dx), CH.cheby_scaffold(O, Ho, 1, 1, 2, 0.3).cycle(np.zeros(b.size), b))
    out = ctx.empty(b.size)
    with pytest.raises(ra.AmgError):  # out of place: x_out must not be x
        A.chebyshev_step(dx, None, to_dev(ctx, b), dx, C1, C2)
    A.chebyshev_step(dx, None, to_dev(ctx, b), out, C1, C2)
