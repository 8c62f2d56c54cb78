"""The numpy restatement of Solver::fgmres (raptor_amd/csrc/multilevel.hip), its case
table and an independently written modified Gram-Schmidt GMRES: tests/test_fgmres_cpu.py checks
them on the CPU, tests/test_gpu_fgmres.py runs the product against the restatement.

fgmres_restated is the definition of include/raptor_amd.h over an oracle hierarchy and the
oracle's residual / spmv, with the dot product left open like bicgstab_cases.bicgstab_restated:
with dot_tree it has the product's c, eta, rotations and y bit for bit.  numpy / scipy only."""
import numpy as np

from tests import bicgstab_cases as B

KRYLOV_OK, KRYLOV_BREAKDOWN = B.KRYLOV_OK, B.KRYLOV_BREAKDOWN
MAX_RESTART = 64
RESTARTS = [1, 2, 3, 5, 30]
FAMS = ["jacobi", "gs"]   # pmis + jacobi, sa + hybrid_gs (cycle_option_cases.FAMILIES)
# (operator key, family): key is (nx, ny, nz, pe) for convdiff or ("chain", n, pe) for upwind_chain
CASES = [(dims + (pe,), fam) for dims in B.GRIDS for pe in B.PES for fam in FAMS]


def operator(key):
    """(row_ptr, col, val) of a case key."""
    return B.upwind_chain(*key[1:]) if key[0] == "chain" else B.convdiff(*key)


def fgmres_restated(H, A, x, b, restart, max_iter, tol, dot, trace=None):
    """Right-preconditioned restarted flexible GMRES, M = H.cycle from zero, one-pass classical
    Gram-Schmidt.  Returns x, the history (||b - A x_0||, then the Arnoldi estimates |g_{j+1}|),
    the iterations counted and the status.  trace (a dict) receives the unrotated Hessenberg
    columns (c_0 .. c_j, eta) of every cycle under "hess" and every x written under "x"."""
    x = np.array(x, np.float64, copy=True)
    n = x.size
    M = lambda v: H.cycle(np.zeros(n), v)  # noqa: E731
    hist = []
    k = 0
    status = KRYLOV_OK
    with np.errstate(all="ignore"):
        while True:
            r = A.residual(x, b)
            beta = np.sqrt(dot(r, r))
            if not hist:
                hist.append(beta)
            if not np.isfinite(beta):
                status = KRYLOV_BREAKDOWN
                break
            if beta == 0.0 or k == max_iter:
                break
            V = [r / beta]
            Z, Hc, g, cs, sn = [], [], [beta], [], []
            raw = []
            stop = False
            while len(Z) < restart and k < max_iter:
                j = len(Z)
                z = M(V[j])
                w = A.spmv(z)
                c = [dot(V[i], w) for i in range(j + 1)]   # all from the same w
                for i in range(j + 1):
                    w = w - c[i] * V[i]
                eta = np.sqrt(dot(w, w))
                h = c + [eta]
                raw.append(list(h))
                for i in range(j):
                    t = cs[i] * h[i] + sn[i] * h[i + 1]
                    h[i + 1] = (-(sn[i] * h[i])) + cs[i] * h[i + 1]
                    h[i] = t
                d = np.sqrt(h[j] * h[j] + h[j + 1] * h[j + 1])
                if d == 0.0 or not np.isfinite(d):
                    status = KRYLOV_BREAKDOWN
                    stop = True
                    raw.pop()
                    break
                cs.append(h[j] / d)
                sn.append(h[j + 1] / d)
                h[j] = d
                g.append(-(sn[j] * g[j]))
                g[j] = cs[j] * g[j]
                Z.append(z)
                Hc.append(h[:j + 1])
                k += 1
                hist.append(abs(g[j + 1]))
                if eta == 0.0:
                    stop = True
                    break
                if tol > 0.0 and hist[0] > 0.0 and hist[k] / hist[0] < tol:
                    stop = True
                    break
                V.append(w / eta)
            J = len(Z)
            y = [np.float64(0.0)] * J
            for i in range(J - 1, -1, -1):
                s = g[i]
                for l in range(i + 1, J):
                    s = s - Hc[l][i] * y[l]
                y[i] = s / Hc[i][i]
            for i in range(J):
                x = x + y[i] * Z[i]
            if trace is not None:
                trace.setdefault("hess", []).append((beta, raw))
                trace.setdefault("x", []).append(x.copy())
            if stop or k == max_iter:
                break
    return x, np.array(hist, np.float64), k, status


def gmres_mgs(H, A, x, b, restart, max_iter, tol):
    """Textbook right-preconditioned GMRES(restart) with modified Gram-Schmidt and numpy's own
    dot, norm and least-squares solve (no rotations): an implementation that shares no line with
    the restatement.  Returns x and the residual estimates (the least-squares residual norms)."""
    x = np.array(x, np.float64, copy=True)
    n = x.size
    r0 = None
    est = []
    k = 0
    while True:
        r = b - A.spmv(x)
        beta = np.linalg.norm(r)
        if r0 is None:
            r0 = beta
            est.append(beta)
        if beta == 0.0 or k == max_iter:
            return x, np.array(est)
        V = np.zeros((restart + 1, n))
        Z = np.zeros((restart, n))
        Hm = np.zeros((restart + 1, restart))
        V[0] = r / beta
        done = False
        j = 0
        while j < restart and k < max_iter and not done:
            Z[j] = H.cycle(np.zeros(n), V[j])
            w = A.spmv(Z[j])
            for i in range(j + 1):          # modified: each coefficient from the w updated so far
                Hm[i, j] = np.dot(V[i], w)
                w = w - Hm[i, j] * V[i]
            Hm[j + 1, j] = np.linalg.norm(w)
            e1 = np.zeros(j + 2)
            e1[0] = beta
            y, *_ = np.linalg.lstsq(Hm[:j + 2, :j + 1], e1, rcond=None)
            res = np.linalg.norm(e1 - Hm[:j + 2, :j + 1] @ y)
            j += 1
            k += 1
            est.append(res)
            if Hm[j, j - 1] == 0.0 or (tol > 0.0 and res / r0 < tol):
                done = True
            else:
                V[j] = w / Hm[j, j - 1]
        x = x + Z[:j].T @ y
        if done or k == max_iter:
            return x, np.array(est)
