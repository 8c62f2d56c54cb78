"""The Chebyshev smoother's restatement (tests/cheby_cases.py) checked on the CPU: the scaffold
against the oracle's own Jacobi cycle, the eigenvalue estimate against the oracle's SA power
iteration, the recurrence against Chebyshev polynomials, and the case tables the GPU tests
(tests/test_gpu_cheby.py) compare the product with.  The last two tests check the built library's
C-ABI and its Python mirror.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from tests import cheby_cases as CH
from tests import cycle_option_cases as K
from tests.edge_cases import bits


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def hierarchies(oracle):
    """(matrix, b, oracle hierarchy) per (problem, family), shared and read only."""
    out = {}
    for kind in K.PROBLEMS:
        for fam in CH.FAMILIES:
            Ao, b, Ho = CH.hierarchy(oracle, kind, fam)
            b.setflags(write=False)
            assert Ho.num_levels >= 4
            out[kind, fam] = (Ao, b, Ho)
    return out


@pytest.mark.parametrize("pre,post,omega", [(1, 1, 2.0 / 3.0), (2, 1, 0.5), (0, 2, 1.0)])
def test_scaffold_with_jacobi_is_the_oracles_cycle(oracle, pre, post, omega):
    """The scaffold with the oracle's Jacobi sweep plugged in is orc_hier_cycle / orc_hier_solve
    bit for bit: what the Chebyshev cycle is restated on."""
    O = oracle
    Ao, b = K.problem(O, "7pt")
    Ho = O.Hierarchy(Ao, **K.oracle_options(O, "jacobi", pre, post, omega))
    S = CH.jacobi_scaffold(O, Ho, pre, post, omega)
    n = b.size
    x, xo = np.zeros(n), np.zeros(n)
    for _ in range(3):
        x, xo = S.cycle(x, b), Ho.cycle(xo, b)
        assert _same(x, xo)
    xs, hs = S.solve(np.zeros(n), b, max_iter=3)
    xo, ho = Ho.solve(np.zeros(n), b, max_iter=3)
    assert _same(xs, xo) and _same(hs, ho)


@pytest.mark.parametrize("kind", list(K.PROBLEMS))
@pytest.mark.parametrize("fam", CH.FAMILIES)
def test_level_eig_is_the_oracles_power_iteration(oracle, hierarchies, kind, fam):
    """lambda_l restated = orc_sa_rho(A_l, diag A_l, seed + l) on every non-coarsest level."""
    O = oracle
    _, _, Ho = hierarchies[kind, fam]
    for l in range(Ho.num_levels - 1):
        A = Ho.matrix(l, "A")
        d = A.diagonal()
        Al = O.Csr.from_scipy(A)
        lam = CH.level_eig(O, Al, d, CH.SEED + l)
        assert _same([lam], [O.sa_rho(Al, d, CH.SEED + l)]), l
        assert 1.0 < lam < 4.0, (l, lam)


def _cheb_T(m, z):
    """T_m(z) by the three-term recurrence."""
    t0, t1 = 1.0, z
    if m == 0:
        return t0
    for _ in range(m - 1):
        t0, t1 = t1, 2.0 * z * t1 - t0
    return t1


@pytest.mark.parametrize("fraction", CH.FRACTIONS)
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6])
def test_recurrence_is_chebyshevs(oracle, m, fraction):
    """On the scalar operator [mu] with b = 0, m steps scale the error by
    T_m((theta - mu) / delta) / T_m(sigma), for mu across [lo, hi] (ten points, none a root of
    T_m for m <= 6) and outside it."""
    O = oracle
    lam = 1.9
    lo, hi, theta, delta, sigma = CH.interval(lam, fraction)
    coef = CH.coefficients(lam, m, fraction)
    worst = 0.0
    for mu in np.concatenate([np.linspace(lo, hi, 10), [0.05 * lo, 0.5 * lo, 1.05 * hi, 1.3 * hi]]):
        A = O.Csr.from_arrays(1, 1, [0, 1], [0], [mu])
        x = CH.cheby_apply(A, np.array([1.0]), coef, np.array([1.0]), np.zeros(1))
        want = _cheb_T(m, (theta - mu) / delta) / _cheb_T(m, sigma)
        assert abs(x[0] - want) <= 1e-12 * abs(want), (mu, x[0], want)
        if lo <= mu <= hi:
            worst = max(worst, abs(x[0]))
    assert worst <= 1.0 / _cheb_T(m, sigma) * (1 + 1e-12)  # the minimax bound on [lo, hi]
    # a step from zero is the same polynomial: x = (1 - p(mu)) b / mu
    A = O.Csr.from_arrays(1, 1, [0, 1], [0], [theta])
    x = CH.cheby_apply(A, np.array([1.0]), coef, np.zeros(1), np.array([theta]), x_zero=True)
    want = 1.0 - _cheb_T(m, 0.0) / _cheb_T(m, sigma)
    assert abs(x[0] - want) <= 1e-12


def test_zero_eigenvalue_gives_zero_coefficients():
    assert CH.coefficients(0.0, 3, 0.3) == (0.0, [0.0] * 3, [0.0] * 3)
    w0, c1, c2 = CH.coefficients(2.0, 1, 0.3)
    assert w0 == 1.0 / (0.5 * (1.1 * 2.0 + 0.3 * (1.1 * 2.0))) and c1 == [0.0] and c2 == [0.0]


@pytest.mark.parametrize("kind", list(K.PROBLEMS))
@pytest.mark.parametrize("fam", CH.FAMILIES)
def test_restated_cycle_converges(oracle, hierarchies, kind, fam):
    """Degrees 1 .. 4 (fraction 0.3, one sweep each side): every one of twelve cycles reduces
    the residual, to less than half of the first in all."""
    O = oracle
    Ao, b, Ho = hierarchies[kind, fam]
    for m in CH.DEGREES:
        S = CH.cheby_scaffold(O, Ho, 1, 1, m, 0.3)
        _, h = S.solve(np.zeros(b.size), b, max_iter=12)
        print(kind, fam, m, "residual reduction per cycle", (h[-1] / h[0]) ** (1.0 / 12))
        assert np.all(np.isfinite(h)) and np.all(h[1:] < h[:-1]), (m, h)
        assert h[-1] < 0.5 * h[0], (m, h[-1] / h[0])


@pytest.mark.parametrize("kind", list(K.PROBLEMS))
def test_every_option_changes_the_iterate(oracle, hierarchies, kind):
    """Every (degree, fraction, pre, post) of the GPU table gives its own cycle (an option the
    restatement ignored would make the GPU comparison vacuous), and the table covers every
    degree and fraction with several (pre, post)."""
    O = oracle
    seen = {}
    for fam, pre, post, m, f in CH.OPTION_CASES:
        _, b, Ho = hierarchies[kind, fam]
        x = CH.cheby_scaffold(O, Ho, pre, post, m, f).cycle(np.zeros(b.size), b)
        assert np.all(np.isfinite(x))
        for key, x2 in seen.items():
            if key[0] == fam:
                assert not np.array_equal(x, x2), ((fam, pre, post, m, f), key)
        seen[fam, pre, post, m, f] = x
    for fam in CH.FAMILIES:
        cs = [c for c in CH.OPTION_CASES if c[0] == fam]
        assert {c[1:3] for c in cs} == set(CH.SWEEPS)
        assert {c[3] for c in cs} == set(CH.DEGREES) and {c[4] for c in cs} == set(CH.FRACTIONS)
        for m in CH.DEGREES:
            assert len({c[1:3] for c in cs if c[3] == m}) >= 2
        one = [c for c in CH.gpu_matrix() if c[1] == "tpl" and c[2] == fam and c[0] == kind]
        assert {c[5] for c in one} == set(CH.DEGREES) and {c[6] for c in one} == set(CH.FRACTIONS)
    assert len(CH.gpu_matrix()) == len(set(CH.gpu_matrix())) <= 100


@pytest.mark.parametrize("fam,what", list(CH.STOP))
def test_stop_index_is_well_defined(oracle, hierarchies, fam, what):
    """The stopping tests' tolerances under Chebyshev (degree 2, fraction 0.3): the restated
    loops stop strictly inside (0, max_iter) and no hist[k] / hist[0] lies within 1 % of tol."""
    O = oracle
    Ao, b, Ho = hierarchies["7pt", fam]
    S = CH.cheby_scaffold(O, Ho, 1, 1, 2, 0.3)
    n = b.size
    tol, max_iter = CH.STOP[fam, what]["tol"], CH.STOP[fam, what]["max_iter"]
    if what == "solve":
        h = S.solve(np.zeros(n), b, max_iter=max_iter, tol=tol)[1]
    else:
        h = np.sqrt(K.pcg_restated(S, Ao, np.zeros(n), b, max_iter, tol, K.dot_tree)[1])
    assert 2 <= len(h) - 1 < max_iter
    ratio = h / h[0]
    assert ratio[-1] < tol and np.all(ratio[:-1] >= tol)
    assert np.all(np.abs(ratio - tol) >= 0.01 * tol), ratio


# ---- the built library and its mirror ---------------------------------------------------------
def test_library_exports_the_chebyshev_entry_points():
    import raptor_amd as ra
    from raptor_amd import _lib

    assert ra.AMG_SMOOTH_CHEBYSHEV == _lib.AMG_SMOOTH_CHEBYSHEV == 2
    raw = C.CDLL(_lib.lib_path)
    for name in ("amg_par_csr_chebyshev_step", "amg_solver_level_eig"):
        assert name in _lib.SIGNATURES
        assert getattr(raw, name) is not None
    assert len(_lib.SIGNATURES["amg_par_csr_chebyshev_step"][1]) == 7
    assert hasattr(ra.ParCSRMatrix, "chebyshev_step") and hasattr(ra.ParMultilevel, "level_eig")
    assert ra.ParMultilevel._SMOOTH["chebyshev"] == 2


def test_options_default_sets_the_chebyshev_fields():
    import raptor_amd as ra
    from raptor_amd import _lib

    names = [f for f, _ in _lib.Options._fields_]
    assert names[-2:] == ["cheby_degree", "cheby_fraction"]
    for preset in (_lib.AMG_PRESET_PMIS_JACOBI, _lib.AMG_PRESET_RS_JACOBI, _lib.AMG_PRESET_SA_HYBRID_GS):
        o = _lib.Options()
        o.cheby_degree, o.cheby_fraction = -7, -1.0
        assert _lib.lib().amg_options_default(preset, C.byref(o)) == 0
        assert o.cheby_degree == 2 and o.cheby_fraction == 0.3
        assert o.smoother != _lib.AMG_SMOOTH_CHEBYSHEV  # the presets' smoothers stay
    ml = ra.ParMultilevel(smoother="chebyshev", cheby_degree=3, cheby_fraction=0.1)
    assert (ml.options.smoother, ml.options.cheby_degree, ml.options.cheby_fraction) == (2, 3, 0.1)
    ml = ra.ParMultilevel()
    assert (ml.options.cheby_degree, ml.options.cheby_fraction) == (2, 0.3)
