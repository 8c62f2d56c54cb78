"""The device setup (setup_device.hip: strength, PMIS, MIS(2), classical interpolation in its
thread and wave forms, SA filtering / rho / smoothing, R = P^T, the drop tolerance) and the
Galerkin SpGEMM (spgemm.hip) on the operators of tests/setup_edge_cases.py: mixed signs,
negative and missing diagonals, s_k == 0, hub rows of 63 .. 600 entries, exact ties, level sizes
around the kernels' block sizes, and SpGEMM rows on every table limit.

tests/test_setup_edges_cpu.py proves on the CPU that each operator reaches the branch it is
built for, that the oracle equals the independent numpy restatement on it, and that a kernel
wrong in that branch would give other bits.  Here every comparison is on bit patterns
(setup_edge_cases.same_bits: a stored -0.0 differs from 0.0); the solve history alone is
compared within the 1e-10 relative of DESIGN.md 3.

Path assertions: the SpGEMM's host-row count is only printed in an AMG_TIMING lap, and that
switch is read once per process, so it cannot be turned on for one test.  A fresh child process
with AMG_TIMING=1 that runs the row_bins product and reads the lap from its stderr was the
alternative; it was not taken, because 8193 distinct columns cannot fit the 8192-slot table
whatever the path, and the row bins rely on the distinct-column counts and bounds the CPU
module proves.

Omissions (the two the cases allow): none.  no_diagonal_neighbour is accepted by from_csr and
by the setup and runs here (setup only: it is never smoothed); amg_par_csr_create accepts a
rank without rows, and test_matmat_ranks runs one."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import setup_edge_cases as E
from tests.setup_edge_cases import same_bits
from tests.test_gpu_multirank import run_ranks
from tests.util import loopback_ctx, to_dev, to_host

pytestmark = pytest.mark.gpu

NPR = {"default": None, "wave": "0", "thread": "1000000"}
SMOOTHER = {"pmis": "jacobi", "sa": "hybrid_gs"}


def _orc(O, M):
    M = sp.csr_matrix(M)
    return O.Csr.from_arrays(M.shape[0], M.shape[1], M.indptr, M.indices, M.data)


def _dev(ra, ctx, M, lo=0, hi=None):
    hi = M.shape[0] if hi is None else hi
    L = M[lo:hi]
    return ra.ParCSRMatrix.from_csr(ctx, M.shape[0], lo, L.indptr, L.indices, L.data)


def _set_npr(monkeypatch, npr):
    if NPR[npr] is None:
        monkeypatch.delenv("AMG_INTERP_WAVE_NPR", raising=False)
    else:
        monkeypatch.setenv("AMG_INTERP_WAVE_NPR", NPR[npr])


_REF = {}


def reference(O, name, kind, drop_tol=0.0):
    """The oracle's hierarchy of a case, computed once and shared (read-only): per level the
    scipy copies of A, P, R, the split, and the oracle's own transpose of P."""
    key = (name, kind, drop_tol)
    if key not in _REF:
        c = E.zoo()[name]
        H = O.Hierarchy(_orc(O, c.A), coarsen=O.COARSEN_PMIS if kind == "pmis" else O.COARSEN_SA,
                        smoother=O.SMOOTH_JACOBI if kind == "pmis" else O.SMOOTH_HYBRID_GS,
                        drop_tol=drop_tol, **getattr(c, kind))
        levels = []
        for l in range(H.num_levels):
            lev = {"A": H.matrix(l, "A")}
            if l + 1 < H.num_levels:
                lev.update(P=H.matrix(l, "P"), R=H.matrix(l, "R"), split=H.split(l))
                lev["PT"] = _orc(O, lev["P"]).transpose().to_scipy()
            levels.append(lev)
        _REF[key] = (H, levels)
    return _REF[key]


def _solver(ra, kind, c, **kw):
    return ra.ParMultilevel(coarsen=kind, smoother=SMOOTHER[kind], **dict(getattr(c, kind), **kw))


def _check_hierarchy(ml, levels, tag):
    assert ml.num_levels == len(levels), (tag, ml.num_levels, len(levels))
    for l, lev in enumerate(levels):
        for w in ("APR" if "P" in lev else "A"):
            assert same_bits(ml.level_matrix(l, w).to_scipy_local(), lev[w]), (tag, l, w)
        if "P" in lev:
            # R is the oracle's transpose of the device's own P (empty P rows, coarse columns
            # used once included)
            assert same_bits(ml.level_matrix(l, "R").to_scipy_local(), lev["PT"]), (tag, l, "P^T")
            assert np.array_equal(ml.level_split(l), lev["split"]), (tag, l, "split")


# ---- one rank: every setup operator, every setup path ------------------------------------------------
ONE_RANK = [(n, k, npr) for n, k in E.setups() for npr in (NPR if k == "pmis" else ["default"])]


@pytest.mark.parametrize("name,kind,npr", ONE_RANK, ids=[f"{n}-{k}-{p}" for n, k, p in ONE_RANK])
def test_setup_one_rank(ctx, oracle, monkeypatch, name, kind, npr):
    """setup_device 1 (device strength, splitting, P, R = P^T), 2 (device Galerkin product only)
    and 0 (host): every level's A, P, R and split equal the oracle's, hence each other's.  PMIS
    operators with the default wave rule, a wave per row everywhere and a thread per row
    everywhere."""
    import raptor_amd as ra

    c = E.zoo()[name]
    _, levels = reference(oracle, name, kind)
    _set_npr(monkeypatch, npr)
    A = _dev(ra, ctx, c.A)
    for m in (1, 2, 0):
        ml = _solver(ra, kind, c, setup_device=m, use_graph=False).setup(A)
        assert (ml.num_levels == 1) if c.one_level else (ml.num_levels >= 2)
        _check_hierarchy(ml, levels, m)
        del ml


def test_checks_notice_one_changed_entry(ctx, oracle):
    """The comparisons are not vacuous on the device side: with 2^-10 added to one a_ik of
    sk_zero (the s_k == 0 neighbour of tile 7's row i, whose value goes into d), the device's P
    differs from the reference in that row and in no other, and R and A_1 differ too."""
    import raptor_amd as ra

    c = E.zoo()["sk_zero"]
    _, levels = reference(oracle, "sk_zero", "pmis")
    i = int(c.claims["rows_i"][7])
    M = c.A.copy()
    k = M.indptr[i] + int(np.searchsorted(M.indices[M.indptr[i]:M.indptr[i + 1]], i + 1))
    assert M.indices[k] == i + 1
    M.data[k] += 2.0 ** -10
    for m in (1, 0):
        ml = _solver(ra, "pmis", c, setup_device=m, use_graph=False).setup(_dev(ra, ctx, M))
        P, Pref = ml.level_matrix(0, "P").to_scipy_local(), levels[0]["P"]
        assert np.array_equal(P.indptr, Pref.indptr) and np.array_equal(P.indices, Pref.indices)
        rows = np.unique(np.searchsorted(P.indptr, np.flatnonzero(E.bits(P.data) != E.bits(Pref.data)), side="right") - 1)
        assert rows.tolist() == [i], (m, rows)
        assert np.array_equal(ml.level_split(0), levels[0]["split"])
        assert not same_bits(ml.level_matrix(0, "R").to_scipy_local(), levels[0]["R"])
        assert not same_bits(ml.level_matrix(1, "A").to_scipy_local(), levels[1]["A"])
        with pytest.raises(AssertionError):
            _check_hierarchy(ml, levels, m)
        del ml


@pytest.mark.parametrize("name,kind", E.setups(), ids=[f"{n}-{k}" for n, k in E.setups()])
def test_galerkin_path(ctx, oracle, name, kind):
    """R.matmat(A.matmat(P)) equals level 1's A and the oracle's R @ (A @ P); with drop_tol 0.01
    and 10 the device's A_1 is the oracle's sparsify of that product (10: a diagonal operator,
    and the coarsening stops there)."""
    import raptor_amd as ra

    O = oracle
    c = E.zoo()[name]
    _, levels = reference(O, name, kind)
    A = _dev(ra, ctx, c.A)
    ml = _solver(ra, kind, c, setup_device=1, use_graph=False).setup(A)
    if c.one_level:
        assert ml.num_levels == 1 == len(levels)
        return
    P, R = ml.level_matrix(0, "P"), ml.level_matrix(0, "R")
    AP = A.matmat(P)
    Ac = R.matmat(AP).to_scipy_local()
    Po, Ro, Ao = _orc(O, levels[0]["P"]), _orc(O, levels[0]["R"]), _orc(O, c.A)
    APo = Ao @ Po
    Aco = Ro @ APo
    assert same_bits(AP.to_scipy_local(), APo.to_scipy())
    assert same_bits(Ac, Aco.to_scipy())
    assert same_bits(Ac, ml.level_matrix(1, "A").to_scipy_local())
    for tol in (0.01, 10.0):
        md = _solver(ra, kind, c, setup_device=1, use_graph=False, drop_tol=tol).setup(A)
        assert md.num_levels >= 2
        A1 = md.level_matrix(1, "A").to_scipy_local()
        assert same_bits(A1, O.sparsify(Aco, tol).to_scipy()), tol
        _check_hierarchy(md, reference(O, name, kind, tol)[1], ("drop", tol))
        if tol == 10.0:
            assert A1.nnz == A1.shape[0] and md.num_levels == 2
        del md


# ---- SpGEMM directly ---------------------------------------------------------------------------------------
_PRODUCTS = {}


def products(O, name):
    """Per pair, computed once: the pure-Python canonical product and the oracle's @."""
    if name not in _PRODUCTS:
        p = E.pairs()[name]
        _PRODUCTS[name] = (E.canonical_product(p.A, p.B), (_orc(O, p.A) @ _orc(O, p.B)).to_scipy())
    return _PRODUCTS[name]


@pytest.mark.parametrize("name", list(E.pairs()))
def test_matmat(ctx, oracle, name):
    """A.matmat(B) on every operand pair: indptr, indices and the bits of the data of the
    canonical-order product and of the oracle's."""
    import raptor_amd as ra

    p = E.pairs()[name]
    Cc, Co = products(oracle, name)
    C = _dev(ra, ctx, p.A).matmat(_dev(ra, ctx, p.B)).to_scipy_local()
    assert same_bits(C, Cc)
    assert same_bits(C, Co)


RANK_PAIRS = [(n, nr, None) for n, p in E.pairs().items() for nr in sorted(p.cuts)] + \
             [("empty_rows", 3, [0, 4, 4]), ("row_bins", 3, [0, 500, 500])]


@pytest.mark.parametrize("name,nranks,cuts", RANK_PAIRS,
                         ids=[f"{n}-{nr}" + ("" if cu is None else "-zero-row-rank") for n, nr, cu in RANK_PAIRS])
def test_matmat_ranks(oracle, name, nranks, cuts):
    """A.matmat(B) on 2 and 3 loopback ranks: every rank's rows of the canonical product.  The
    row_bins cuts leave rank 0 without a halo and make the 8192- and 8193-column rows read
    ghost rows of B; nnz_a_0 and nnz_b_0 run with no halo on any rank, a zero-length ghost-row
    exchange and an empty B image; the last two cases hold a rank without rows."""
    import raptor_amd as ra

    p = E.pairs()[name]
    Cc, _ = products(oracle, name)
    n = p.A.shape[0]
    starts = list(p.cuts[nranks] if cuts is None else cuts) + [n]

    def rank(r, nr, world):
        ctx = loopback_ctx(r, nr, world)
        lo, hi = starts[r], starts[r + 1]
        A, B = _dev(ra, ctx, p.A, lo, hi), _dev(ra, ctx, p.B, lo, hi)
        return A.info["n_halo"], A.matmat(B).to_scipy_local()

    res = run_ranks(nranks, rank)
    for r, (halo, C) in enumerate(res):
        assert same_bits(C, Cc[starts[r]:starts[r + 1]]), r
    if name == "row_bins":
        assert res[0][0] == 0 and res[-1][0] > 0


# ---- several loopback ranks: the setup -------------------------------------------------------------------
RANK_SETUPS = [(n, k, nr) for n, k in E.setups() if E.zoo()[n].cuts for nr in sorted(E.zoo()[n].cuts)]


@pytest.mark.parametrize("name,kind,nranks", RANK_SETUPS, ids=[f"{n}-{k}-{nr}" for n, k, nr in RANK_SETUPS])
def test_setup_ranks(oracle, name, kind, nranks):
    """from_csr on a ragged partition whose cuts pass through hub neighbourhoods and gadget
    tiles (strong F neighbours become ghost rows, strong C neighbours halo points),
    replicate_below = 0, setup_device 1 and 0: every rank's rows of every level's A, P, R and
    split are the serial oracle's."""
    import raptor_amd as ra

    c = E.zoo()[name]
    _, levels = reference(oracle, name, kind)
    n = c.A.shape[0]
    starts = list(c.cuts[nranks]) + [n]

    def rank(r, nr, world):
        ctx = loopback_ctx(r, nr, world)
        A = _dev(ra, ctx, c.A, starts[r], starts[r + 1])
        out = []
        for m in (1, 0):
            ml = _solver(ra, kind, c, setup_device=m, replicate_below=0, use_graph=False).setup(A)
            lev = []
            for l in range(ml.num_levels):
                d = {}
                for w in ("APR" if l + 1 < ml.num_levels else "A"):
                    M = ml.level_matrix(l, w)
                    d[w] = (M.first_row, M.to_scipy_local())
                if l + 1 < ml.num_levels:
                    d["split"] = ml.level_split(l)
                lev.append(d)
            out.append(lev)
            del ml
        return out

    for r, per_mode in enumerate(run_ranks(nranks, rank)):
        for m, lev in zip((1, 0), per_mode):
            assert len(lev) == len(levels) >= 2, (r, m)
            for l, d in enumerate(lev):
                for w in ("APR" if "P" in d else "A"):
                    f, M = d[w]
                    assert same_bits(M, levels[l][w][f:f + M.shape[0]]), (r, m, l, w)
                if "split" in d:
                    f, M = d["A"]
                    assert np.array_equal(d["split"], levels[l]["split"][f:f + M.shape[0]]), (r, m, l)


# ---- one end-to-end check: the edge hierarchies are usable ---------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", ["pmis", "sa"])
@pytest.mark.parametrize("name", ["mixed_2500", "hub"])
def test_cycles_on_edge_hierarchies(ctx, oracle, name, kind, graph):
    """PMIS + Jacobi and SA + hybrid GS: four cycles bit-identical to the oracle's cycle on the
    oracle's own hierarchy, a four-cycle solve history within 1e-10 relative, and the residual
    going down."""
    import raptor_amd as ra

    c = E.zoo()[name]
    Ho, levels = reference(oracle, name, kind)
    A = _dev(ra, ctx, c.A)
    ml = _solver(ra, kind, c, use_graph=graph).setup(A)
    assert ml.graph_enabled == graph
    _check_hierarchy(ml, levels, "cycle")
    n = c.A.shape[0]
    b = _orc(oracle, c.A).spmv(oracle.vec_uniform(n, 42))
    db, dx, xo = to_dev(ctx, b), ctx.zeros(n), np.zeros(n)
    for it in range(4):
        ml.cycle(dx, db)
        xo = Ho.cycle(xo, b)
        assert np.array_equal(E.bits(to_host(ctx, dx)), E.bits(xo)), it
    _, hist = ml.solve(ctx.zeros(n), db, max_iter=4)
    _, hist_o = Ho.solve(np.zeros(n), b, max_iter=4)
    assert hist.size == hist_o.size == 5
    assert np.all(np.abs(hist - hist_o) <= 1e-10 * hist_o)
    assert hist[-1] < hist[0]
