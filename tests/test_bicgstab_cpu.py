"""BiCGStab on the CPU: the restatement of tests/bicgstab_cases.py (the loop Solver::bicgstab is
held to bit for bit by tests/test_gpu_bicgstab.py) converges on convection-diffusion operators
where the oracle's PCG does not, the product's host setup equals the oracle's on those
operators, the breakdown rule, and the new call's place in the interface.  No GPU needed."""
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import bicgstab_cases as B
from tests import cycle_option_cases as K
from tests.util import same_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMS = ["jacobi", "gs"]   # pmis + jacobi, sa + hybrid_gs (cycle_option_cases.FAMILIES)
TOL, CAP = 1e-8, 15


def _problem(O, dims, pe):
    csr = B.convdiff(*dims, pe)
    Ao = B.oracle_matrix(O, csr)
    return csr, Ao, B.rhs(O, Ao.shape[0])


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("pe", B.PES)
@pytest.mark.parametrize("dims", B.GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_restatement_converges(oracle, dims, pe, fam):
    """1e-8 in at most 15 iterations on the product's dot tree, status OK, the recorded norm is
    the true one; three ragged ranks' dot products change the run by rounding only.  No history
    ratio lies within 1 % of the tolerance, so a history that agrees to a few digits (the
    device's sqrt) stops at the same iteration."""
    O = oracle
    _, Ao, b = _problem(O, dims, pe)
    n = b.size
    Ho = O.Hierarchy(Ao, **K.oracle_options(O, fam, max_coarse=B.MAX_COARSE))
    assert Ho.num_levels >= 3
    x, rr, st = B.bicgstab_restated(Ho, Ao, np.zeros(n), b, CAP, TOL, K.dot_tree)
    h = np.sqrt(rr)
    assert st == B.KRYLOV_OK
    assert 1 < len(h) <= CAP + 1 and h[-1] / h[0] < TOL and np.all(h[:-1] / h[0] >= TOL)
    assert np.all(np.abs(h / h[0] / TOL - 1.0) > 0.01)
    true = O.norm2(Ao.residual(x, b))
    assert abs(h[-1] - true) <= 1e-6 * true
    cuts = B.ragged_cuts(n, 3)
    xc, rrc, stc = B.bicgstab_restated(Ho, Ao, np.zeros(n), b, CAP, TOL,
                                       lambda u, v: K.dot_tree(u, v, cuts))
    assert stc == B.KRYLOV_OK and abs(len(rrc) - len(rr)) <= 1
    assert np.sqrt(rrc[-1]) / np.sqrt(rrc[0]) < TOL
    m = min(len(rr), len(rrc)) - 1   # the histories agree while both run (rounding only)
    assert np.allclose(np.sqrt(rrc[:m]), h[:m], rtol=1e-6, atol=0)
    assert np.allclose(xc, x, rtol=0, atol=1e-6 * np.abs(x).max())


@pytest.mark.parametrize("pe", [0.5, 8.0])
@pytest.mark.parametrize("dims", B.GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_pcg_does_not_cover_the_ground(oracle, dims, pe):
    """The oracle's PCG (pmis + jacobi) is not at 1e-8 after 40 iterations on these operators."""
    O = oracle
    _, Ao, b = _problem(O, dims, pe)
    Ho = O.Hierarchy(Ao, **K.oracle_options(O, "jacobi", max_coarse=B.MAX_COARSE))
    with np.errstate(all="ignore"):
        _, h = Ho.pcg(np.zeros(b.size), b, max_iter=40, tol=TOL)
    assert len(h) == 41 and not h[-1] / h[0] < TOL, h


# name: (product options, oracle defaults, extended+i)
SETUPS = {"classical": (dict(coarsen="pmis"), "pmis", False),
          "ext+i": (dict(coarsen="pmis", interp="ext+i", p_max=4), "pmis", True),
          "sa": (dict(coarsen="sa"), "sa", False)}


@pytest.mark.parametrize("setup", list(SETUPS))
@pytest.mark.parametrize("pe", [0.5, 8.0])
@pytest.mark.parametrize("dims", B.GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_host_setup_equals_oracle_on_nonsymmetric_operators(oracle, dims, pe, setup):
    from raptor_amd import host

    O = oracle
    (rp, col, val), Ao, _ = _problem(O, dims, pe)
    pkw, coarsen, ext = SETUPS[setup]
    okw = dict(interp=O.INTERP_EXT_I, p_max=4) if ext else {}
    Hp = host.HostHierarchy(Ao.shape[0], 0, rp, col, val, host.options(max_coarse=B.MAX_COARSE, **pkw))
    Ho = O.Hierarchy(Ao, **dict(O.DEFAULTS[coarsen], max_coarse=B.MAX_COARSE, **okw))
    assert Hp.num_levels == Ho.num_levels >= 3
    for l in range(Ho.num_levels):
        assert same_csr(Hp.to_scipy(l, "A"), Ho.matrix(l, "A")), l
        if l + 1 < Ho.num_levels:
            assert same_csr(Hp.to_scipy(l, "P"), Ho.matrix(l, "P")), l
            assert same_csr(Hp.to_scipy(l, "R"), Ho.matrix(l, "R")), l
            assert np.array_equal(Hp.split(l), Ho.split(l)), l
    assert not same_csr(Ho.matrix(0, "A"), Ho.matrix(0, "A").T)   # the operator is nonsymmetric


def test_exact_start_is_a_breakdown_that_leaves_x(oracle):
    """b = A x0: r = 0, so rhat.v = 0 in the first iteration: nothing is written or counted."""
    O = oracle
    _, Ao, _ = _problem(O, B.GRIDS[1], 2.0)
    n = Ao.shape[0]
    Ho = O.Hierarchy(Ao, **K.oracle_options(O, "jacobi", max_coarse=B.MAX_COARSE))
    x0 = np.rint(8 * O.vec_uniform(n, 3))   # small integers: A x0 and the residual are exact
    b = Ao.spmv(x0)
    assert not np.any(Ao.residual(x0, b))
    x, rr, st = B.bicgstab_restated(Ho, Ao, x0, b, 10, 0.0, K.dot_tree)
    assert st == B.KRYLOV_BREAKDOWN and rr.tolist() == [0.0] and np.array_equal(x, x0)


def one_level_problem(O):
    """convdiff(5, 3, 2, 2.0), 30 rows under max_coarse = 32: the cycle is the coarse solve, so
    BiCGStab runs on (almost) the identity and runs out of residual."""
    csr = B.convdiff(5, 3, 2, 2.0)
    Ao = B.oracle_matrix(O, csr)
    Ho = O.Hierarchy(Ao, **K.oracle_options(O, "jacobi", max_coarse=B.MAX_COARSE))
    return csr, Ao, Ho, B.rhs(O, Ao.shape[0])


def test_one_level_run_ends_in_a_breakdown_with_x_finite(oracle):
    O = oracle
    _, Ao, Ho, b = one_level_problem(O)
    assert Ho.num_levels == 1
    trace = []
    x, rr, st = B.bicgstab_restated(Ho, Ao, np.zeros(b.size), b, 10, 0.0, K.dot_tree, trace)
    assert st == B.KRYLOV_BREAKDOWN and len(rr) - 1 == len(trace) < 10
    assert all(np.all(np.isfinite(t)) for t in trace) and np.array_equal(x, trace[-1])
    assert np.all(np.isfinite(rr))
    true = O.norm2(Ao.residual(x, b))
    assert true <= 1e-12 * np.sqrt(rr[0])   # the last iterate written solves the system


def test_interface():
    import raptor_amd as ra
    from raptor_amd import _lib

    assert len(_lib.SIGNATURES["amg_solver_bicgstab"][1]) == 8
    assert (_lib.AMG_KRYLOV_OK, _lib.AMG_KRYLOV_BREAKDOWN) == (0, 1)
    assert (ra.AMG_KRYLOV_OK, ra.AMG_KRYLOV_BREAKDOWN) == (0, 1)
    sig = inspect.signature(ra.ParMultilevel.bicgstab)
    assert list(sig.parameters) == ["self", "x", "b", "max_iter", "tol"]
    assert sig.parameters["max_iter"].default == 20 and sig.parameters["tol"].default == 0.0
    hdr = open(os.path.join(ROOT, "include", "raptor_amd.h")).read()
    assert "#define AMG_KRYLOV_OK 0" in hdr and "#define AMG_KRYLOV_BREAKDOWN 1" in hdr


def test_cxx_facade_has_bicgstab(tmp_path):
    src = tmp_path / "facade.cpp"
    src.write_text('#include "raptor_amd.hpp"\n'
                   'int main() { return &raptor_amd::ParMultilevel::bicgstab == nullptr; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-address",
                        "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
