"""FGMRES on the CPU: the restatement of tests/fgmres_cases.py (the loop Solver::fgmres is held to
bit for bit by tests/test_gpu_fgmres.py) converges for every restart of the table, counts what an
independent modified Gram-Schmidt GMRES counts, reports an estimate that is the true residual
norm, rotates correctly, handles the exact cases, and has its place in the interface.  No GPU."""
import fnmatch
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bicgstab_cases as B
from tests import cycle_option_cases as K
from tests import fgmres_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, CAP = 1e-8, 40
# the largest ||b - A x|| / hist[-1] at the stop over CASES x RESTARTS (test_estimate_is_the_
# true_residual prints each): the bar is twice this
WORST_TRUE_OVER_ESTIMATE = 1.000000002342

_SETUP = {}


def _setup(O, key, fam):
    """(oracle matrix, hierarchy, b) of a case, built once."""
    if (key, fam) not in _SETUP:
        Ao = B.oracle_matrix(O, G.operator(key))
        Ho = O.Hierarchy(Ao, **K.oracle_options(O, fam, max_coarse=B.MAX_COARSE))
        b = B.rhs(O, Ao.shape[0])
        b.setflags(write=False)
        _SETUP[key, fam] = (Ao, Ho, b)
    return _SETUP[key, fam]


_RUNS = {}


def _run(O, key, fam, restart):
    """The restatement on dot_tree at tol 1e-8, cap 40, once per (case, restart)."""
    k = (key, fam, restart)
    if k not in _RUNS:
        Ao, Ho, b = _setup(O, key, fam)
        _RUNS[k] = G.fgmres_restated(Ho, Ao, np.zeros(b.size), b, restart, CAP, TOL, K.dot_tree)
    return _RUNS[k]


def _id(case):
    key, fam = case
    return "-".join(map(str, key)) + "-" + fam


@pytest.mark.parametrize("restart", G.RESTARTS)
@pytest.mark.parametrize("case", G.CASES, ids=_id)
def test_restatement_converges(oracle, case, restart):
    """1e-8 inside 40 iterations for every restart, status OK, the estimate falls monotonically
    inside a cycle, and no history ratio lies within 1 % of the tolerance (so a history that
    agrees to a few digits stops at the same iteration)."""
    x, h, k, st = _run(oracle, *case, restart)
    assert st == G.KRYLOV_OK and 1 < k < CAP and len(h) == k + 1
    assert h[-1] / h[0] < TOL and np.all(h[:-1] / h[0] >= TOL)
    assert np.all(np.abs(h / h[0] / TOL - 1.0) > 0.01)
    for c0 in range(0, k, restart):   # inside a cycle |g_{j+1}| = |sn_j| |g_j| <= |g_j|
        seg = h[c0 + 1:c0 + restart + 1]
        assert np.all(np.diff(seg) <= 0.0)


@pytest.mark.parametrize("case", G.CASES, ids=_id)
def test_restart_30_counts_what_mgs_counts_and_no_more_cycles_than_bicgstab(oracle, case):
    """One-pass classical Gram-Schmidt loses nothing here: the count is the modified
    Gram-Schmidt / least-squares implementation's; and at one cycle per iteration against
    BiCGStab's two, FGMRES never spends more cycles."""
    O = oracle
    Ao, Ho, b = _setup(O, *case)
    x, h, k, st = _run(O, *case, 30)
    xm, hm = G.gmres_mgs(Ho, Ao, np.zeros(b.size), b, 30, CAP, TOL)
    assert len(hm) - 1 == k
    assert np.allclose(hm, h, rtol=1e-6, atol=0)
    assert np.allclose(xm, x, rtol=0, atol=1e-9 * np.abs(x).max())
    _, rr, stb = B.bicgstab_restated(Ho, Ao, np.zeros(b.size), b, CAP, TOL, K.dot_tree)
    assert stb == B.KRYLOV_OK and np.sqrt(rr[-1] / rr[0]) < TOL
    assert k <= 2 * (len(rr) - 1)


def test_estimate_is_the_true_residual(oracle):
    """||b - A x|| at the stop over hist[-1], the Arnoldi estimate, for every case and restart of
    the table.  Measured on the restatement (not the product) over the 12 x 5 runs: smallest
    0.999999992997 (12x11x10, pe 0.5, sa + gs, restart 30), largest 1.000000002342 (12x11x10, pe
    8, sa + gs, restart 2).  The bar is twice the largest."""
    O = oracle
    worst = 0.0
    for case in G.CASES:
        Ao, Ho, b = _setup(O, *case)
        for restart in G.RESTARTS:
            x, h, k, st = _run(O, *case, restart)
            ratio = O.norm2(Ao.residual(x, b)) / h[-1]
            print("%s restart %d: k = %d, true / estimate = %.12f" % (_id(case), restart, k, ratio))
            worst = max(worst, ratio)
    assert worst <= 2.0 * WORST_TRUE_OVER_ESTIMATE, worst


@pytest.mark.parametrize("case", [G.CASES[1], G.CASES[-2]], ids=_id)
def test_rotations_give_the_least_squares_residual(oracle, case):
    """Eight steps in one cycle: |g_{k+1}| of the Givens recurrence equals the residual norm of
    min ||beta e_1 - Hbar_k y|| over the unrotated Hessenberg, from numpy.linalg.lstsq."""
    O = oracle
    Ao, Ho, b = _setup(O, *case)
    trace = {}
    x, h, k, st = G.fgmres_restated(Ho, Ao, np.zeros(b.size), b, 30, 8, 0.0, K.dot_tree, trace)
    assert k == 8 and st == G.KRYLOV_OK and len(trace["hess"]) == 1
    beta, cols = trace["hess"][0]
    assert beta == h[0] and len(cols) == 8
    Hbar = np.zeros((9, 8))
    for j, col in enumerate(cols):
        Hbar[:j + 2, j] = col
    for kk in range(1, 9):
        e1 = np.zeros(kk + 1)
        e1[0] = beta
        y, *_ = np.linalg.lstsq(Hbar[:kk + 1, :kk], e1, rcond=None)
        res = np.linalg.norm(e1 - Hbar[:kk + 1, :kk] @ y)
        print("step %d: |g| = %.17g, lstsq = %.17g, rel = %.2e" % (kk, h[kk], res, abs(h[kk] - res) / res))
        assert abs(h[kk] - res) <= 1e-12 * res


def test_one_by_one_is_a_happy_breakdown(oracle):
    """n = 1, A = [4], b = [3]: M is exact, w = v_0, c_0 = 1 and eta == 0 exactly: one
    iteration, hist = [3, 0], x = 0.75, status OK -- and the later limit is never reached."""
    import scipy.sparse as sp

    O = oracle
    A1 = O.Csr.from_scipy(sp.csr_matrix(np.array([[4.0]])))
    H1 = O.Hierarchy(A1, **K.oracle_options(O, "jacobi", max_coarse=B.MAX_COARSE))
    for tol in (0.0, 1e-8):
        x, h, k, st = G.fgmres_restated(H1, A1, np.zeros(1), np.array([3.0]), 5, 4, tol, K.dot_tree)
        assert (k, st, h.tolist(), x.tolist()) == (1, G.KRYLOV_OK, [3.0, 0.0], [0.75])


def test_exact_start_and_zero_limit_leave_x(oracle):
    """b = A x0 in integers: r = 0, no iteration, hist = [0], status OK, x untouched.  max_iter =
    0: hist = [beta], x untouched."""
    O = oracle
    Ao, Ho, b = _setup(O, B.GRIDS[1] + (0.5,), "jacobi")
    n = b.size
    x0 = np.rint(8 * O.vec_uniform(n, 3))   # small integers: A x0 and the residual are exact
    bx = Ao.spmv(x0)
    assert not np.any(Ao.residual(x0, bx))
    for tol in (0.0, 1e-8):
        x, h, k, st = G.fgmres_restated(Ho, Ao, x0, bx, 5, 10, tol, K.dot_tree)
        assert (k, st, h.tolist()) == (0, G.KRYLOV_OK, [0.0]) and np.array_equal(x, x0)
    x, h, k, st = G.fgmres_restated(Ho, Ao, x0, b, 5, 0, 0.0, K.dot_tree)
    r = Ao.residual(x0, b)
    assert (k, st) == (0, G.KRYLOV_OK) and h.tolist() == [np.sqrt(K.dot_tree(r, r))]
    assert np.array_equal(x, x0)


def test_interface():
    """The header, the export list and the Python mirror all carry amg_solver_fgmres; the Python
    method has the documented signature and defaults."""
    import raptor_amd as ra
    from raptor_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "raptor_amd.h")).read()
    assert "#define AMG_FGMRES_MAX_RESTART 64" in hdr
    assert re.search(r"\bint amg_solver_fgmres\(amg_solver S, double\* x, const double\* b, int32_t restart, "
                     r"int32_t max_iter,\s+double tol, double\* hist, int32_t\* iters, int32_t\* status\);", hdr)
    emap = open(os.path.join(ROOT, "raptor_amd", "csrc", "exports.map")).read()
    exported = re.search(r"global:(.*?)local:", emap, re.S).group(1).replace(";", " ").split()
    assert any(fnmatch.fnmatchcase("amg_solver_fgmres", pat) for pat in exported)
    assert len(_lib.SIGNATURES["amg_solver_fgmres"][1]) == 9
    sig = inspect.signature(ra.ParMultilevel.fgmres)
    assert list(sig.parameters) == ["self", "x", "b", "max_iter", "tol", "restart"]
    assert [sig.parameters[p].default for p in ("max_iter", "tol", "restart")] == [20, 0.0, 30]
    assert G.MAX_RESTART == 64


def test_cxx_facade_has_fgmres(tmp_path):
    src = tmp_path / "facade.cpp"
    src.write_text('#include "raptor_amd.hpp"\n'
                   'int main() { return &raptor_amd::ParMultilevel::fgmres == nullptr; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-address",
                        "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
