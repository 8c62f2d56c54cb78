"""The restatement of tests/mc_gs_cases.py checked on the CPU: the colouring is proper on
A u A^T, is first-fit in key order and does not depend on how the ids are cut into ranks; the
sweep's fixed point is the solution; the restated cycle needs no more than 0.7 x hybrid GS's
cycles on the two smoothed-aggregation workloads; the library exports the entry points."""
import ctypes as C

import numpy as np
import pytest

from tests import mc_gs_cases as M
from tests import setup_edge_cases as SE

_OPS = {}


def _ops(O):
    if not _OPS:
        _OPS.update(M.operators(O))
        assert list(_OPS) == M.OPERATORS
    return _OPS


_COLOURS = {}


def _colours(O, name):
    if name not in _COLOURS:
        c, r = M.first_fit(_ops(O)[name], M.SEED)
        c.setflags(write=False)
        _COLOURS[name] = (c, r)
    return _COLOURS[name]


@pytest.mark.parametrize("name", M.OPERATORS)
def test_colouring_is_proper_on_a_union_at(oracle, name):
    A = _ops(oracle)[name].tocoo()
    c, _ = _colours(oracle, name)
    assert c.min() >= 0
    off = A.row != A.col
    assert np.all(c[A.row[off]] != c[A.col[off]])  # each stored entry: both directions of A u A^T


@pytest.mark.parametrize("name", M.OPERATORS)
def test_colouring_is_first_fit(oracle, name):
    """Every vertex holds the smallest colour its preceding neighbours leave free: none of them
    has its colour, and each smaller colour is used by one of them."""
    A = _ops(oracle)[name]
    c, _ = _colours(oracle, name)
    rp, col = M.adjacency(A)
    n = A.shape[0]
    key = SE.hash32(np.arange(n), M.SEED).astype(np.int64)
    for v in range(n):
        nb = col[rp[v]:rp[v + 1]]
        before = nb[(key[nb] > key[v]) | ((key[nb] == key[v]) & (nb < v))]
        assert set(c[before].tolist()) >= set(range(c[v])), v
        assert c[v] not in set(c[before].tolist()), v


@pytest.mark.parametrize("nranks", [1, 2, 3])
@pytest.mark.parametrize("name", M.OPERATORS)
def test_colouring_is_equal_under_cuts(oracle, name, nranks):
    """Rank by rank in parallel readiness rounds (each rank sees the others' colours of the
    previous round only): the sequential loop's colours, in the sequential loop's round count."""
    A = _ops(oracle)[name]
    c, r = _colours(oracle, name)
    cc, rr = M.first_fit_cut(A, M.SEED, M.cuts(A.shape[0], nranks))
    assert np.array_equal(cc, c) and rr == r


def test_case_list_holds_what_it_claims(oracle):
    ops = _ops(oracle)
    A = ops["upwind_lower"]
    assert (A != A.T).nnz > 0 and sp_pattern_asymmetric(A) and not sp_pattern_asymmetric(ops["upwind_chain"])
    assert np.abs(ops["convdiff"] - ops["convdiff"].T).max() > 0 and not sp_pattern_asymmetric(ops["convdiff"])
    for name in ("single_row_colours", "wave_colours"):
        c, _ = _colours(oracle, name)
        assert np.any(np.bincount(c) == 1), name
    # a colour whose rows average more than a slice's width, and its rows end inside a round of 64
    c, _ = _colours(oracle, "wave_colours")
    A = ops["wave_colours"]
    lens = np.diff(A.indptr)
    avg = np.bincount(c, weights=lens) / np.bincount(c)
    assert np.any(avg > M.SLICE) and np.any(avg <= M.SLICE)
    assert np.any((lens > M.SLICE) & (lens % M.SLICE != 0))
    assert _colours(oracle, "hub")[0].max() + 1 >= 6
    # keys fall along the path: the rounds run as long as a stretch, where 7-pt needs a dozen
    assert _colours(oracle, "path")[1] >= SE.PATH_RUN
    for n in (M.SLICE - 1, M.SLICE, M.SLICE + 1):
        assert ops[f"rows_{n}"].shape[0] == n


def sp_pattern_asymmetric(A):
    P = A.copy()
    P.data = np.ones_like(P.data)
    return (P != P.T).nnz > 0


@pytest.mark.parametrize("name", M.OPERATORS)
def test_sweep_fixed_point_is_the_solution(oracle, name):
    """With b = A x a sweep in either direction returns x itself, and from another start repeated
    sweeps move towards it."""
    O = oracle
    A = _ops(O)[name]
    Ao = O.Csr.from_scipy(A)
    c, _ = _colours(O, name)
    n = A.shape[0]
    xs = O.vec_uniform(n, 11)
    b = Ao.spmv(xs)
    # b_i is the very sum row_dot forms (CSR order, no FMA), so b_i - s = 0.0 in every row a sweep
    # visits: x stays, bit for bit
    for back in (False, True):
        assert np.array_equal(M.sweep(Ao, c, xs, b, back).view(np.uint64), xs.view(np.uint64))
    # Gauss-Seidel on these diagonally dominant operators contracts the error
    x = np.zeros(n)
    e0 = np.max(np.abs(x - xs))
    for _ in range(30):
        x = M.sweep(Ao, c, x, b)
    assert np.max(np.abs(x - xs)) < 0.5 * e0


def test_sweep_is_a_gauss_seidel_sweep_in_colour_order(oracle):
    """Against a row-by-row Gauss-Seidel loop over the rows sorted by colour (any order inside a
    colour gives the same bits: rows of one colour never read each other)."""
    O = oracle
    A = _ops(O)["27pt"]
    Ao = O.Csr.from_scipy(A)
    c, _ = _colours(O, "27pt")
    n = A.shape[0]
    x0, b = O.vec_uniform(n, 5), O.vec_uniform(n, 6)
    d = A.diagonal()
    for back in (False, True):
        x = x0.copy()
        order = np.argsort(c, kind="stable")
        if back:
            order = order[::-1]
        for i in order:
            s = 0.0
            for k in range(A.indptr[i], A.indptr[i + 1]):
                s += A.data[k] * x[A.indices[k]]
            x[i] = x[i] + (1.0 / d[i]) * (b[i] - s)
        assert np.array_equal(x.view(np.uint64), M.sweep(Ao, c, x0, b, back).view(np.uint64))


# ---- the condition: no more than 0.7 x hybrid GS's cycles ------------------------------------------
# The shapes were fixed after checking that the reference alone meets the bar: sa27 24^3 takes 87
# hybrid-GS cycles (block 64) and 35 restated multicolour cycles to 1e-8 (0.40), the 120^2
# substitute (RCM order, drop_tol 0.005) 96 and 57 (0.59).
@pytest.mark.parametrize("what", ["sa27-24", "g3sub-120"])
def test_restated_cycle_needs_at_most_0p7_of_hybrid_gs_cycles(oracle, what):
    O = oracle
    if what == "sa27-24":
        (Ao, b), kw = M.sa27(O, 24), {}
    else:
        (Ao, b), kw = M.g3sub(O, 120), dict(drop_tol=0.005)
    Ho = M.hierarchy(O, Ao, "sa", **kw)
    assert Ho.num_levels >= 3
    _, h = Ho.solve(np.zeros(b.size), b, max_iter=400, tol=1e-8)   # the oracle's own hybrid GS, B = 64
    gs = len(h) - 1
    assert h[-1] / h[0] < 1e-8
    S = M.mc_scaffold(O, Ho)
    mc = M.cycles_to(S, b, 1e-8)
    print(what, "hybrid GS", gs, "multicolour", mc, "ratio", mc / gs, "colours",
          [int(c.max()) + 1 for c in S.colour], "rounds", S.rounds)
    assert mc <= 0.7 * gs, (mc, gs)


# ---- the built library and its mirror ---------------------------------------------------------
def test_library_exports_the_multicolour_entry_points():
    import raptor_amd as ra
    from raptor_amd import _lib

    assert ra.AMG_SMOOTH_MC_GS == _lib.AMG_SMOOTH_MC_GS == 3
    raw = C.CDLL(_lib.lib_path)
    for name in ("amg_par_csr_colour", "amg_par_csr_colours", "amg_par_csr_mc_gs", "amg_solver_level_colours"):
        assert name in _lib.SIGNATURES
        assert getattr(raw, name) is not None
    assert len(_lib.SIGNATURES["amg_par_csr_mc_gs"][1]) == 5
    for m in ("colour", "colours", "mc_gs"):
        assert hasattr(ra.ParCSRMatrix, m)
    assert hasattr(ra.ParMultilevel, "level_colours") and ra.ParMultilevel._SMOOTH["mc_gs"] == 3
    # the byte model is the last field of amg_matrix_info; amg_options is unchanged
    assert [f for f, _ in _lib.MatrixInfo._fields_][-1] == "mc_gs_bytes"
    assert [f for f, _ in _lib.Options._fields_][-2:] == ["cheby_degree", "cheby_fraction"]
    ml = ra.ParMultilevel(smoother="mc_gs")
    assert ml.options.smoother == 3
    for preset in (_lib.AMG_PRESET_PMIS_JACOBI, _lib.AMG_PRESET_RS_JACOBI, _lib.AMG_PRESET_SA_HYBRID_GS):
        o = _lib.Options()
        assert _lib.lib().amg_options_default(preset, C.byref(o)) == 0
        assert o.smoother != _lib.AMG_SMOOTH_MC_GS  # defaults and presets stay
