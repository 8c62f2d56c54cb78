"""The Chebyshev smoother (AMG_SMOOTH_CHEBYSHEV) restated for the tests: the
coefficient recurrence in Python floats, the eigenvalue estimate and the steps on the oracle's
kernels with numpy elementwise operations, and a V-cycle scaffold over an oracle hierarchy's
exported A, P and R (the hierarchy does not depend on the smoother).  tests/test_cheby_cpu.py
anchors the scaffold on the oracle's own Jacobi cycle; tests/test_gpu_cheby.py runs the product
against it.  Every operation is one rounded fp64 operation, in the order the definition writes."""
import numpy as np

from tests import cycle_option_cases as K
from tests.golden.gen_golden import coarse_solve

EIG_ITERS = 10     # power steps of lambda_l
BOOST = 1.1        # hi = 1.1 lambda_l
SEED = 0x5EED      # amg_options.seed's default (lambda_l is seeded with seed + l)

DEGREES = [1, 2, 3, 4]
FRACTIONS = [0.3, 0.1]
SWEEPS = [(1, 1), (0, 1), (1, 0), (2, 1), (2, 2)]
FAMILIES = ["pmis", "sa"]
# (degree, fraction) in an order whose every window of six holds all four degrees and both
# fractions: the rotation below starts one further along for each (pre, post)
DEGREE_FRACTION = [(1, 0.3), (2, 0.1), (3, 0.3), (4, 0.1), (1, 0.1), (2, 0.3), (3, 0.1), (4, 0.3)]


def _rotated(values, width):
    """cycle_option_cases._rotated's rule over this module's SWEEPS."""
    return [(pre, post) + values[(i + k) % len(values)]
            for i, (pre, post) in enumerate(SWEEPS) for k in range(width)]


# (family, pre, post, degree, fraction)
OPTION_CASES = [(fam,) + c for fam in FAMILIES for c in _rotated(DEGREE_FRACTION, 2)]


def gpu_matrix():
    """(kind, env, family, pre, post, degree, fraction): the option table as built, and one
    (degree, fraction) per (pre, post) -- another rotation -- without the row templates' floor."""
    one = [(fam,) + c for fam in FAMILIES for c in _rotated(DEGREE_FRACTION[::-1], 1)]
    out = []
    for kind in K.PROBLEMS:
        out += [(kind, "built") + c for c in OPTION_CASES]
        out += [(kind, "tpl") + c for c in one]
    return out


def case_id(c):
    *head, fam, pre, post, m, f = c
    return "-".join([*head, fam, f"{pre}{post}", f"m{m}", f"f{f}"])


# ---- the definition ------------------------------------------------------------------------------
def coefficients(lam, degree, fraction):
    """(w0, c1, c2): c1[k], c2[k] for step k >= 1 (entry 0 unused).  lam = 0: all 0.0."""
    c1, c2 = [0.0] * degree, [0.0] * degree
    if lam == 0.0:
        return 0.0, c1, c2
    hi = BOOST * lam
    lo = fraction * hi
    theta = 0.5 * (hi + lo)
    delta = 0.5 * (hi - lo)
    sigma = theta / delta
    w0 = 1.0 / theta
    rho = 1.0 / sigma
    for k in range(1, degree):
        rk = 1.0 / (2.0 * sigma - rho)
        c1[k] = rk * rho
        c2[k] = (2.0 * rk) / delta
        rho = rk
    return w0, c1, c2


def interval(lam, fraction):
    """(lo, hi, theta, delta, sigma) of coefficients()."""
    hi = BOOST * lam
    lo = fraction * hi
    theta = 0.5 * (hi + lo)
    delta = 0.5 * (hi - lo)
    return lo, hi, theta, delta, theta / delta


def level_eig(O, A, d, seed):
    """rho(D^-1 A) by SA's power iteration on A itself: A an oracle Csr, d its
    diagonal.  x = u / max|u|; y = (A x) / d; lam = max|y|; x = y / lam; stop at lam = 0."""
    x = O.vec_uniform(A.shape[0], seed)
    m = np.max(np.abs(x), initial=0.0)
    if m > 0.0:
        x = x / m
    lam = 0.0
    for _ in range(EIG_ITERS):
        y = A.spmv(x) / d
        lam = float(np.max(np.abs(y), initial=0.0))
        if lam == 0.0:
            break
        x = y / lam
    return lam


def cheby_step(A, dinv, x, xprev, b, c1, c2):
    """One step k >= 1: x' = x + ((c1 (x - xprev)) + (c2 (dinv (b - A x))))."""
    t = A.residual(x, b)
    u = x - xprev
    v = dinv * t
    w = (c1 * u) + (c2 * v)
    return x + w


def cheby_apply(A, dinv, coef, x, b, x_zero=False):
    """One application of degree m = len(c1).  x_zero: step 0 is w0 (dinv b), as the product's
    Jacobi sweep from zero, and the iterate before it is 0.0 in every row."""
    w0, c1, c2 = coef
    if x_zero:
        prev, cur = np.zeros(b.size), w0 * (dinv * b)
    else:
        prev, cur = x, x + w0 * (dinv * A.residual(x, b))
    for k in range(1, len(c1)):
        prev, cur = cur, cheby_step(A, dinv, cur, prev, b, c1[k], c2[k])
    return cur


# ---- the V-cycle scaffold ------------------------------------------------------------------------
class Scaffold:
    """cycle / solve of the oracle (cycle_rec, orc_hier_solve) over exported level operators,
    with the smoother left open: smoother(l, x, b, x_zero, post) -> the smoothed x."""

    def __init__(self, O, Ho, smoother=None):
        self.O = O
        self.nl = Ho.num_levels
        self.A = [O.Csr.from_scipy(Ho.matrix(l, "A")) for l in range(self.nl)]
        self.P = [O.Csr.from_scipy(Ho.matrix(l, "P")) for l in range(self.nl - 1)]
        self.R = [O.Csr.from_scipy(Ho.matrix(l, "R")) for l in range(self.nl - 1)]
        self.diag = [Ho.matrix(l, "A").diagonal() for l in range(self.nl)]
        self.inv = O.dense_inverse(self.A[-1])
        self.pre = self.post = 1
        self.smoother = smoother

    def _rec(self, l, x, b, x_zero):
        if l == self.nl - 1:
            return coarse_solve(self.inv, b)
        for _ in range(self.pre):
            x = self.smoother(l, x, b, x_zero, False)
            x_zero = False
        r = self.A[l].residual(x, b)
        bc = self.R[l].spmv(r)
        xc = self._rec(l + 1, np.zeros(bc.size), bc, True)
        x = self.P[l].spmv_add(xc, x)
        for _ in range(self.post):
            x = self.smoother(l, x, b, False, True)
        return x

    def cycle(self, x, b):
        return self._rec(0, np.array(x, np.float64), np.ascontiguousarray(b, np.float64), False)

    def solve(self, x, b, max_iter=10, tol=0.0):
        O = self.O
        hist = [O.norm2(self.A[0].residual(x, b))]
        it = 0
        while it < max_iter:
            x = self.cycle(x, b)
            hist.append(O.norm2(self.A[0].residual(x, b)))
            it += 1
            if hist[0] > 0.0 and hist[-1] / hist[0] < tol:
                break
        return x, np.array(hist)


def jacobi_scaffold(O, Ho, pre, post, omega):
    S = Scaffold(O, Ho)
    S.pre, S.post = pre, post
    S.smoother = lambda l, x, b, x_zero, post_: S.A[l].jacobi(x, b, omega)
    return S


def cheby_scaffold(O, Ho, pre, post, degree, fraction, seed=SEED):
    """The restated Chebyshev hierarchy over Ho's operators; .lam: lambda_l per smoothed level."""
    S = Scaffold(O, Ho)
    S.pre, S.post = pre, post
    S.lam = [level_eig(O, S.A[l], S.diag[l], seed + l) for l in range(S.nl - 1)]
    S.coef = [coefficients(lam, degree, fraction) for lam in S.lam]
    S.dinv = [1.0 / d for d in S.diag[:-1]]
    S.smoother = lambda l, x, b, x_zero, post_: cheby_apply(S.A[l], S.dinv[l], S.coef[l], x, b, x_zero)
    return S


def hierarchy(O, kind, fam):
    """(oracle matrix, b, oracle hierarchy) of a section-3 problem; the smoother is irrelevant."""
    Ao, b = K.problem(O, kind)
    return Ao, b, O.Hierarchy(Ao, **dict(O.DEFAULTS[fam], max_coarse=K.MAX_COARSE))


def product_options(fam, pre=1, post=1, degree=2, fraction=0.3, max_coarse=K.MAX_COARSE):
    return dict(coarsen=fam, smoother="chebyshev", pre_sweeps=pre, post_sweeps=post,
                cheby_degree=degree, cheby_fraction=fraction, max_coarse=max_coarse)


# ---- stopping rules (7-pt problem, degree 2, fraction 0.3, one solver per family) ---------------
STOP = {
    ("pmis", "solve"): dict(tol=1e-4, max_iter=40),
    ("sa", "solve"): dict(tol=1e-6, max_iter=40),
    ("pmis", "pcg"): dict(tol=1e-8, max_iter=40),
    ("sa", "pcg"): dict(tol=1e-10, max_iter=40),
}


def bytes_model(infos, l, pre, post, degree):
    """Solver::bytes_per_cycle under Chebyshev, from n, nnz and the sizes of P and R
    (infos[l] = level_info(l)): step 0 costs what a Jacobi sweep costs there, each later step
    base + 40 n; copy back iff (pre + post) degree is odd."""
    inf = infos[l]
    n, nnz = inf["n_local"], inf["nnz_local"]
    if l + 1 == len(infos):
        cn = inf["n_global"]
        return 8 * cn * n + 8 * cn + 8 * n
    nc = infos[l + 1]["n_local"]
    base = 12 * nnz + 4 * (n + 1)
    later = (degree - 1) * (base + 40 * n)
    total, zero = 0, l > 0
    for _ in range(pre):
        total += 24 * n if zero else base + 32 * n
        total += later
        zero = False
    if zero:
        total += 8 * n
    total += base + 24 * n
    total += 12 * inf["r_nnz_local"] + 4 * (nc + 1) + 8 * n + 8 * nc
    total += 12 * inf["p_nnz_local"] + 4 * (n + 1) + 8 * nc + 8 * n + 8 * n
    total += post * (base + 32 * n + later)
    if (pre + post) * degree % 2 == 1:
        total += 16 * n
    return total
